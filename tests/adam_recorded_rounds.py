"""Child process of tests/test_hip_adam_trainer.py: runs its recorded-against-eager rounds (``_run_recorded_rounds``, every trainer with
``adam="native"``, ``graphs=True``, ``head_update="bf16"``) with the convolution library in DETERMINISTIC mode and writes SHA-256 digests of
both nets' parameters and the optimizers' step counts as JSON to ``sys.argv[1]``.

Why a process of its own: as tests/head_recorded_rounds.py -- the library's deterministic mode depends on environment variables that the
library reads once per process, so they are set here before anything is imported."""
import hashlib
import json
import os
import sys

for _v in ("FWD", "BWD", "WRW"):
    os.environ[f"MIOPEN_DEBUG_CONV_DIRECT_NAIVE_CONV_{_v}"] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub in ("tests", "oracle", "ipp-marl_amd"):
    sys.path.insert(0, os.path.join(ROOT, sub))

import torch  # noqa: E402

torch.backends.cudnn.deterministic = True


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def main():
    import test_hip_adam_trainer as T
    nets, before, counts = T._run_recorded_rounds()
    out = {net: {"digests": [digest(t) for t in trio], "numel": int(trio[0].numel()),
                 "finite": bool(all(torch.isfinite(t).all() for t in trio)),
                 "premise_differ": int((trio[0] != trio[1]).sum()),
                 "differ": int((trio[0] != trio[2]).sum()), "max": float((trio[0] - trio[2]).abs().max()),
                 "moved": float((trio[0] - before[net]).abs().max())}
           for net, trio in nets.items()}
    with open(sys.argv[1], "w") as f:
        json.dump({"nets": out, "counts": counts}, f)


if __name__ == "__main__":
    main()
