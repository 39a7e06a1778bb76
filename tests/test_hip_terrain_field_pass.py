"""The whole-field form of the terrain's second transform pass (csrc/terrain.hip, k_terrain_fft_y_field: one workgroup per env holds
all rows of a 128- or 256-cell field in registers, reduces the field's (min, max) inside the workgroup and thresholds the rows it
holds) against the library's own reference form: ``ippm_terrain_field`` (the field written out, (min, max) by atomics) followed by
``ippm_terrain_pack`` with its keys -- documented as the same arithmetic, and it has no batch threshold and no knob.

``ippm_terrain_truth`` takes the whole-field form for batches of FIELD_MIN_ENVS envs or more (TERRAIN_FIELD_MIN_ENVS in
csrc/terrain.hip: one workgroup per env fills the device's 256 CUs from there) when both sides are 128 or 256 cells; smaller
batches and larger sides keep the two-pass form.  The whole-field form also decides the threshold bit without the reference's
division (``f - lo >= span / 2`` for ``(f - lo) / span >= 0.5f``, exact for spans within [2^-100, 2^100]), so every comparison here
is one of the two expressions as well.  Everything is compared bit for bit."""
import numpy as np
import pytest

from configs import make_params

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

FIELD_MIN_ENVS = 128     # TERRAIN_FIELD_MIN_ENVS of csrc/terrain.hip


def _world(x, y):
    return dict(environment__x_dim=x, environment__y_dim=y)


# (grid_x, grid_y): config name, overrides
SHAPES = {
    (128, 128): ("small", {}),
    (256, 256): ("c2", {}),
    (128, 256): ("small", _world(50, 100)),
    (256, 128): ("small", _world(100, 50)),
    (512, 512): ("c4", {}),
}


class Synth:
    """One library context on the grid of ``shape`` and a generator of its own: ``truth(ids)`` is ippm_terrain_truth for any batch,
    ``reference(ids)`` the field form + pack."""

    def __init__(self, shape):
        from ippmarl.terrain import RandomFieldTerrain
        from ippmarl.vec_env import VecEnv
        name, over = SHAPES[shape]
        params = make_params(name, experiment__missions__n_agents=2, **over)
        self.env = VecEnv(params, 1, track_area=False, terrain="random_field")
        assert (self.env.d.grid_x, self.env.d.grid_y) == shape
        self.gen = RandomFieldTerrain(self.env.d, self.env.ctx, self.env.device, params["sensor"]["simulation"]["cluster_radius"])
        assert self.gen.native

    def _planes(self, n):
        return torch.zeros((n,) + tuple(self.env.truth.shape[1:]), dtype=self.env.truth.dtype, device=self.env.device)

    def truth(self, ids):
        """-> (packed truth planes [n, bytes], range keys [n, 2]) of ippm_terrain_truth"""
        ep = torch.as_tensor(np.asarray(ids), dtype=torch.int64).to(self.env.device)
        out = self._planes(len(ids))
        self.gen.generate(ep, out, self.env.stream)
        keys = self.gen._keys.view(-1)[: 4 * len(ids)].view(len(ids), 4)[:, :2].clone()
        return out, keys

    def reference(self, ids):
        from ippmarl import _ffi
        env, n = self.env, len(ids)
        gx, gy = env.d.grid_x, env.d.grid_y
        ep = torch.as_tensor(np.asarray(ids), dtype=torch.int64).to(env.device)
        work = torch.empty(n, gy // 2 + 1, gx, 2, dtype=torch.float32, device=env.device)
        field = torch.empty(n, gx, gy, dtype=torch.float32, device=env.device)
        keys = torch.zeros(n, 2, dtype=torch.int32, device=env.device)
        env.ctx.call("ippm_terrain_field", _ffi.ptr(ep), _ffi.ptr(self.gen.amp), None, _ffi.ptr(work), _ffi.ptr(field), _ffi.ptr(keys), n,
                     env.stream)
        out = self._planes(n)
        env.ctx.call("ippm_terrain_pack", _ffi.ptr(field), _ffi.ptr(keys), _ffi.ptr(out), n, env.stream)
        return out, keys


@pytest.mark.parametrize("shape", [(128, 128), (256, 256), (128, 256), (256, 128)])
def test_whole_field_form_equals_the_field_form(shape):
    """Batches of FIELD_MIN_ENVS, FIELD_MIN_ENVS + 1 and 3 FIELD_MIN_ENVS + 5 envs (the threshold, an odd count, more workgroups than
    the device holds at once at 256^2) and one just below the threshold (the two-pass form): truth planes and both range keys equal
    the reference's; the smaller batches are prefixes of the largest one's episode ids, so env e's plane and keys are also shown not
    to depend on the batch (nor on the form) they were generated in."""
    s = Synth(shape)
    big = 3 * FIELD_MIN_ENVS + 5
    ids = np.arange(1, big + 1) * 7919 + 11
    ref_truth, ref_keys = s.reference(ids)
    assert int(ref_truth.max()) > 0 and int(ref_truth.min()) < 255 and not torch.equal(ref_truth[0], ref_truth[1])   # fields, not constants
    for n in (big, FIELD_MIN_ENVS, FIELD_MIN_ENVS + 1, FIELD_MIN_ENVS - 1):
        got, keys = s.truth(ids[:n])
        assert torch.equal(got, ref_truth[:n]), (shape, n)
        assert torch.equal(keys, ref_keys[:n]), (shape, n)


def test_spans_outside_the_direct_range_keep_the_quotient():
    """The whole-field form thresholds without the division only for 2^-100 <= max - min <= 2^100 (terrain_bit in csrc/terrain.hip);
    amplitudes scaled by 2^-112 and 2^112 (exact scalings of the same spectrum) put the span outside on either side: same planes
    and keys as the reference, which always divides."""
    s = Synth((256, 256))
    ids = np.arange(1, FIELD_MIN_ENVS + 2) * 613
    amp = s.gen.amp.clone()
    for scale in (2.0 ** -112, 2.0 ** 112):
        s.gen.amp.copy_(amp * scale)
        ref_truth, ref_keys = s.reference(ids)
        span = ref_keys.cpu().numpy().astype(np.uint32)
        span = (np.where(span & 0x80000000, span & 0x7FFFFFFF, ~span).astype(np.uint32)).view(np.float32)
        span = span[:, 1].astype(np.float64) - span[:, 0]
        assert np.all(span < 2.0 ** -100) or np.all(span > 2.0 ** 100), (scale, span.min(), span.max())
        got, keys = s.truth(ids)
        assert torch.equal(got, ref_truth) and torch.equal(keys, ref_keys), scale
        assert int(got.max()) > 0 and int(got.min()) < 255


def test_side_512_keeps_the_two_pass_form_and_its_result():
    """512 cells a side at a batch above the threshold: served by the two-pass form, same result as the reference."""
    s = Synth((512, 512))
    ids = np.arange(1, FIELD_MIN_ENVS + 2) * 104729
    ref_truth, ref_keys = s.reference(ids)
    got, keys = s.truth(ids)
    assert torch.equal(got, ref_truth) and torch.equal(keys, ref_keys)


def test_two_resets_in_a_row_leave_nothing_behind():
    """VecEnv.reset on config 2's parameters (4 UAVs, 256^2) at a batch that takes the whole-field form, twice with different
    episode ids on the same scratch: ``truth`` is the reference's both times."""
    from ippmarl.vec_env import VecEnv
    n = FIELD_MIN_ENVS + 1
    env = VecEnv(make_params("c2"), n, track_area=False, terrain="random_field")
    s = Synth((256, 256))
    for rep in range(2):
        ids = np.arange(1, n + 1) * 31 + 1000 * rep
        env.reset(ids)
        ref_truth, _ = s.reference(ids)
        assert torch.equal(env.truth, ref_truth), rep
    first, _ = s.reference(np.arange(1, n + 1) * 31)
    assert not torch.equal(env.truth, first)
