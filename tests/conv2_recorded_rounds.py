"""Child process of tests/test_hip_conv2_train.py: runs its recorded-against-eager round (``_run_recorded_round``, both trainers with
``conv2_update="bf16"``) with the convolution library in DETERMINISTIC mode and writes SHA-256 digests of both nets' parameters as JSON to
``sys.argv[1]``.

Why a process of its own: as tests/critic_recorded_rounds.py -- the library's default float32 weight-gradient kernels (conv1's, still the
library's under the switch) sum with float atomics, and its deterministic mode depends on environment variables that the library reads
once per process, so they are set here before anything is imported."""
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
    import test_hip_conv2_train as T
    nets, before = T._run_recorded_round()
    out = {net: {"digests": [digest(t) for t in pair], "numel": int(pair[0].numel()),
                 "finite": bool(all(torch.isfinite(t).all() for t in pair)),
                 "differ": int((pair[0] != pair[1]).sum()), "max": float((pair[0] - pair[1]).abs().max()),
                 "moved": float((pair[0] - before[net]).abs().max())}
           for net, pair in nets.items()}
    with open(sys.argv[1], "w") as f:
        json.dump(out, f)


if __name__ == "__main__":
    main()
