"""Child process of tests/test_hip_critic_native.py: runs its recorded-against-eager rounds (``_run_recorded_rounds``) with the convolution
library in DETERMINISTIC mode and writes SHA-256 digests of the resulting buffers and parameters as JSON to ``sys.argv[1]``.

Why a process of its own: the library's default float32 weight-gradient kernels sum with float atomics, so two launch-by-launch rounds
from the same bits differ in the last bits and a bit-for-bit comparison of a replayed round says nothing.  Its deterministic mode
(``torch.backends.cudnn.deterministic``) needs the library's plain direct convolutions, which ippmarl.networks switches off for speed
through environment variables that the library reads once per process -- so they are set here before anything is imported."""
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
    import test_hip_critic_native as T
    out = []
    for r in T._run_recorded_rounds():
        out.append({"bufs": {k: [digest(b[k]) for b in r["bufs"]] for k in r["bufs"][0]},
                    "nets": {net: {"digests": [digest(t) for t in trio], "numel": int(trio[0].numel()),
                                   "finite": bool(all(torch.isfinite(t).all() for t in trio)),
                                   "differ_recorded": int((trio[0] != trio[2]).sum()), "differ_eager": int((trio[0] != trio[1]).sum()),
                                   "max_recorded": float((trio[0] - trio[2]).abs().max()), "max_eager": float((trio[0] - trio[1]).abs().max()),
                                   "moved": float((trio[0] - r["before"][net]).abs().max())}
                             for net, trio in r["nets"].items()}})
    with open(sys.argv[1], "w") as f:
        json.dump(out, f)


if __name__ == "__main__":
    main()
