"""The input planes of the InstanceNorm budget tests (tests/test_ref64.py on the CPU, tests/test_instancenorm_budget_gpu.py on the GPU): one generator, so
that the measuring stick is proven on the very planes the kernels then see.  Every family is built to be adverse to one way of taking a plane's
statistics in fp32: a mean far from zero in units of the deviation (a sum of squares cancels), a first sample far from the mean (a pivot taken from it
cancels), a sparse plane behind a ReLU (most samples equal, a few carry the variance), no variance at all, a variance far below eps, and neighbouring
channels of very different kinds (a channel lane that reads its neighbour's statistics)."""
import numpy as np

# name -> fp32 only?  (fp16 keeps its values inside the half range: no mean at 1000 deviations)
FAMILIES = {"benign": False, "mean30": False, "mean1000": True, "pivot10": False, "pivot100": False, "sparse": False, "constant": False, "tiny": False, "mixed": False}


def families(dtype):
    return [f for f, f32_only in FAMILIES.items() if not (f32_only and dtype == "f16")]


def _h(a):
    return np.asarray(a, np.float32).astype(np.float16).astype(np.float32)


def plane(family, shape, dtype="f32", seed=0):
    """x [N,H,W,C] float32 (rounded to half first where dtype is "f16"), read-only."""
    n, h, w, c = shape
    r = np.random.default_rng(1000 + seed)
    g = lambda: r.standard_normal(shape)
    if family == "benign":
        x = 0.7 + 1.2 * g()
    elif family == "mean30":
        x = 30.0 + g()
    elif family == "mean1000":
        x = 1000.0 + g()
    elif family in ("pivot10", "pivot100"):
        x = 0.05 * g()
        x[:, 0, 0, :] = 10.0 if family == "pivot10" else 100.0
    elif family == "sparse":
        x = np.maximum(g() - 2.0, 0.0)
        x[:, 0, 0, :] = 6.0
    elif family == "constant":
        x = np.broadcast_to(r.uniform(-4.0, 4.0, (n, 1, 1, c)), shape).copy()
    elif family == "tiny":  # std 1e-4: var = 1e-8 against eps = 1e-5 (around 2e-3, where the spacing of half is 2e-6)
        x = 2e-3 + 1e-4 * g()
    elif family == "mixed":  # even channels constant, odd channels wide
        x = np.where(np.arange(c) % 2 == 0, np.broadcast_to(r.uniform(-4.0, 4.0, (n, 1, 1, c)), shape), 0.3 + 5.0 * g())
    else:
        raise ValueError(family)
    x = np.ascontiguousarray(x, dtype=np.float32)
    if dtype == "f16":
        x = _h(x)
    x.setflags(write=False)
    return x


def params(c, seed=0):
    """(beta, gamma) per channel: gamma in +-[0.5, 1.5], the last channel's negative (C >= 2) and channel 1's zero (C >= 3)."""
    r = np.random.default_rng(2000 + seed)
    beta, gamma = r.uniform(-0.5, 0.5, c).astype(np.float32), r.uniform(0.5, 1.5, c).astype(np.float32)
    if c >= 2:
        gamma[c - 1] = -gamma[c - 1]
    if c >= 3:
        gamma[1] = 0.0
    return beta, gamma
