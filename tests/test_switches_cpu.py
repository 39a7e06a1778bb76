"""CPU checks of the switch table (ippmarl.switches): every row resolves the same way -- the argument, else the environment variable, else
the default -- through the table and through the resolver that keeps the switch's old name, and the trainer's list is the table's."""
import pytest

from ippmarl import switches


def _resolver(name):
    """The resolver of switch ``name`` under the name it had before the table, with its module's constants."""
    from ippmarl import actor_native, critic_native, metrics_native, networks, optim_native, replay_native, rollout_native, shuffle_native
    if name.endswith("_update"):
        up = name.upper()
        return getattr(networks, f"resolve_{name}"), getattr(networks, f"{up}_ENV"), getattr(networks, f"{up}_MODES")
    module = {"rollout_log": rollout_native, "metrics": metrics_native, "buffer": replay_native, "actor_inference": actor_native,
              "critic_inference": critic_native, "adam": optim_native, "shuffle": shuffle_native}[name]
    return module.resolve_mode, module.ENV_VAR, module.MODES


@pytest.mark.parametrize("name", list(switches.TABLE))
def test_every_row_resolves_argument_then_environment_then_default(monkeypatch, name):
    row = switches.TABLE[name]
    old, env_var, modes = _resolver(name)
    assert env_var == row.env_var and modes == row.modes and row.default == row.modes[0] and len(row.modes) == 2
    other = row.modes[1]
    for resolve in (lambda v=None: switches.resolve(name, v), old):
        monkeypatch.delenv(row.env_var, raising=False)
        assert resolve() == row.default and resolve(None) == row.default
        assert resolve(other) == other
        monkeypatch.setenv(row.env_var, other)
        assert resolve() == other                                   # the environment wins over the default
        assert resolve(row.default) == row.default                  # the argument wins over the environment
        monkeypatch.setenv(row.env_var, "")
        assert resolve() == row.default                             # an empty variable means the default
        for bad in ("hip", other.capitalize(), "1"):
            with pytest.raises(ValueError, match=f"^{row.noun} must be one of "):
                resolve(bad)
            monkeypatch.setenv(row.env_var, bad)
            with pytest.raises(ValueError, match=f"^{row.noun} must be one of "):
                resolve()
            assert resolve(other) == other


def test_trainer_lists_the_table():
    from ippmarl.trainer import COMATrainer
    assert COMATrainer.SWITCHES == tuple(switches.TABLE)
    assert COMATrainer.SWITCHES == ("rollout_log", "metrics", "buffer", "actor_inference", "critic_inference", "adam", "head_update",
                                    "conv2_update", "trunk_update", "shuffle")
    assert len({row.env_var for row in switches.TABLE.values()}) == 10
