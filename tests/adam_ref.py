"""The native Adam step's arithmetic contract (include/ippmarl.h) restated in NumPy, once in float32 -- every
operation rounded on its own, in the contract's order: what the kernel must give bit for bit -- and once in float64, whose distance to the
float32 restatement (the "spread") is the unit of every tolerance.  Never the code under test."""
import numpy as np

from actor_native_ref import MARGIN  # noqa: F401  (the project's tolerance unit: MARGIN spreads)

BETAS = (0.9, 0.999)
EPS = 1e-8


class Adam:
    """State and step of one set of tensors.  dtype float32: the contract; float64: the same formulas without any rounding to float32."""

    def __init__(self, params, lr, dtype, betas=BETAS, eps=EPS):
        self.dtype = np.dtype(dtype)
        self.p = [np.array(p, dtype=self.dtype) for p in params]
        self.m = [np.zeros_like(p) for p in self.p]
        self.v = [np.zeros_like(p) for p in self.p]
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self.t, self.b1p, self.b2p = 0, 1.0, 1.0          # (Python floats are doubles)

    def step(self, grads):
        f = self.dtype.type
        b1, b2 = self.betas
        self.b1p *= b1
        self.b2p *= b2
        self.t += 1
        step = f(self.lr / (1.0 - self.b1p))
        rs = f(np.sqrt(1.0 - self.b2p))
        w1, w2, B2, E = f(1.0 - b1), f(1.0 - b2), f(b2), f(self.eps)
        with np.errstate(all="ignore"):
            for i, g in enumerate(grads):
                g = np.asarray(g, dtype=self.dtype)
                m, v, p = self.m[i], self.v[i], self.p[i]
                m = m + w1 * (g - m)
                v = B2 * v + w2 * (g * g)
                den = np.sqrt(v) / rs + E
                p = p - step * (m / den)
                assert m.dtype == v.dtype == p.dtype == self.dtype
                self.m[i], self.v[i], self.p[i] = m, v, p
        return self


def gradients(seed, shapes, zeros=0.1):
    """The input family of the tests: magnitudes 10^U(-12, 3), random signs, ``zeros`` of the elements exactly 0 (float32)."""
    rng = np.random.default_rng(seed)
    out = []
    for shape in shapes:
        g = 10.0 ** rng.uniform(-12.0, 3.0, size=shape) * rng.choice([-1.0, 1.0], size=shape)
        g[rng.random(size=shape) < zeros] = 0.0
        out.append(g.astype(np.float32))
    return out


def parameters(seed, shapes, scale=0.05):
    rng = np.random.default_rng(seed)
    return [(scale * rng.standard_normal(size=shape)).astype(np.float32) for shape in shapes]


def spreads(a32: Adam, a64: Adam):
    """max |float32 restatement - float64 restatement| over all tensors, for p, m and v."""
    def worst(x32, x64):
        return max(float(np.max(np.abs(a.astype(np.float64) - b))) for a, b in zip(x32, x64))
    return {"p": worst(a32.p, a64.p), "m": worst(a32.m, a64.m), "v": worst(a32.v, a64.v)}


def errors(got, a64: Adam):
    """max |got - float64 restatement| for {"p": [...], "m": [...], "v": [...]} of arrays."""
    return {k: max(float(np.max(np.abs(np.asarray(a, dtype=np.float64) - b))) for a, b in zip(got[k], getattr(a64, k))) for k in got}
