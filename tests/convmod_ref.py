"""Reference for the conv module core (csrc/convmod.hip): no GPU code in here.

Written from the contract in include/onebit_hip.h ("Conv module core"): rows = Bt*T frames,
channel fastest, utterance b = rows [b*T, (b+1)*T), P stacked passes of B = Bt/P utterances.

    g = u[:, :C] * sigmoid(u[:, C:])
    z[b, t, c] = sum_j w_dw[c, j] * g[b, t + j - K//2, c] + b_dw[c]     (frames outside [0, T): 0)
    mean[p, c], rstd[p, c] over pass p's B*T rows (biased variance, eps inside the root)
    v = swish(gamma * (z - mean) * rstd + beta),  swish(y) = y * sigmoid(y)

Plain torch on CPU tensors in the dtype of the inputs (float64 for the reference, float32 to
measure what the number format alone costs). The depthwise conv is a sum of K shifted slices
and BatchNorm is written out, so a one-row pass (variance exactly 0) is defined. Gradients
come from autograd on (v * dv).sum().

The case tables of the GPU test live here too, so that the CPU tests can check every case's
conditioning without importing a GPU test module.
"""
from __future__ import annotations

import functools

import torch


def core(u, w_dw, b_dw, gamma, beta, P, T, eps):
    """(v, z, g, mean, rstd): v, z, g [rows, C]; mean, rstd [P, C]. b_dw None: no bias."""
    rows, c2 = u.shape
    C = c2 // 2
    K = w_dw.shape[-1]
    w = w_dw.reshape(C, K)
    Bt = rows // T
    g = u[:, :C] * torch.sigmoid(u[:, C:])
    h = K // 2
    gp = torch.zeros(Bt, T + 2 * h, C, dtype=u.dtype)
    gp[:, h:h + T] = g.view(Bt, T, C)
    z = torch.zeros(Bt, T, C, dtype=u.dtype)
    for j in range(K):
        z = z + w[:, j] * gp[:, j:j + T]
    if b_dw is not None:
        z = z + b_dw
    z = z.reshape(rows, C)
    zp = z.reshape(P, rows // P, C)
    mean = zp.mean(dim=1)
    var = ((zp - mean[:, None]) ** 2).mean(dim=1)
    rstd = 1.0 / torch.sqrt(var + eps)
    y = (zp - mean[:, None]) * rstd[:, None] * gamma + beta
    v = y * torch.sigmoid(y)
    return v.reshape(rows, C), z, g, mean, rstd


def run(t, dtype=torch.float64, bias=True):
    """Forward and autograd backward of `core` on the inputs `t` (see `inputs`) in `dtype`.
    Returns a dict: v, z, g, mean, rstd, du, dw_dw, db_dw, dgamma, dbeta, and dz = dL/dz."""
    P, T, eps = t["P"], t["T"], t["eps"]
    leaf = {k: t[k].to(dtype).clone().requires_grad_(True) for k in ("u", "w", "b", "gamma", "beta")}
    v, z, g, mean, rstd = core(leaf["u"], leaf["w"], leaf["b"] if bias else None, leaf["gamma"],
                               leaf["beta"], P, T, eps)
    z.retain_grad()
    (v * t["dv"].to(dtype)).sum().backward()
    out = {"v": v, "z": z, "g": g, "mean": mean, "rstd": rstd, "du": leaf["u"].grad,
           "dw_dw": leaf["w"].grad, "dgamma": leaf["gamma"].grad, "dbeta": leaf["beta"].grad,
           "db_dw": leaf["b"].grad if bias else torch.zeros_like(leaf["b"]), "dz": z.grad}
    return {k: x.detach() for k, x in out.items()}


def eps_of(K):
    """BatchNorm's eps per case. K = 1 runs with 1e-12: z = w * g + b there, BatchNorm cancels
    the per-channel scale w and dw_dw is a true zero -- but only up to eps / var(z), which at
    the usual 1e-5 is a real gradient, not round-off. (The value is the float32 that the C
    ABI receives, as a Python float.)"""
    return torch.tensor(1e-12 if K == 1 else 1e-5, dtype=torch.float32).item()


@functools.lru_cache(maxsize=None)
def inputs(P, B, T, C, K, variant="std"):
    """float32 CPU inputs, seeded on the CPU, shared and never modified. Pass p's rows of u
    are u * (p + 1) + 0.5 * p, so every pass has its own mean and variance per channel.
    Variants: "awkward" (one gamma 0, one negative, one channel's depthwise weights 0 so that
    its z is the constant bias), "saturated" (a tenth of u from {-100, -88.5, -30, 30, 100})."""
    gen = torch.Generator().manual_seed(100003 * C + 1009 * T + 101 * K + 11 * B + P)
    rows = P * B * T
    u = torch.randn(rows, 2 * C, generator=gen)
    scale = (torch.arange(P, dtype=torch.float32) + 1).repeat_interleave(B * T)[:, None]
    u = u * scale + 0.5 * (scale - 1)
    w = torch.randn(C, K, generator=gen) / K ** 0.5
    b = torch.randn(C, generator=gen) * 0.1
    gamma = torch.rand(C, generator=gen) + 0.5
    beta = torch.randn(C, generator=gen) * 0.2
    dv = torch.randn(rows, C, generator=gen)
    info = {}
    if variant == "awkward":
        i0, i1, i2 = 0, C // 2, C - 1  # three different channels (C >= 3)
        gamma[i0] = 0.0
        gamma[i1] = -gamma[i1]
        w[i2] = 0.0
        # a dyadic bias: the sum of any number of copies is exact in float32 too, so the mean
        # is the bias itself and xhat = 0 does not hinge on the precision of the statistics
        # (1/sqrt(eps) = 316 would multiply whatever the mean is off by)
        b[i2] = -0.25
        info = {"gamma0": i0, "gamma_neg": i1, "const": i2}
    elif variant == "saturated":
        vals = torch.tensor([-100.0, -88.5, -30.0, 30.0, 100.0])
        n = u.numel()
        pos = torch.randperm(n, generator=gen)[: n // 10]
        u.view(-1)[pos] = vals[torch.randint(0, 5, (n // 10,), generator=gen)]
    else:
        assert variant == "std", variant
    return {"u": u, "w": w, "b": b, "gamma": gamma, "beta": beta, "dv": dv, "P": P, "B": B, "T": T,
            "C": C, "K": K, "eps": eps_of(K), "info": info}


@functools.lru_cache(maxsize=None)
def reference(P, B, T, C, K, variant="std", bias=True):
    """float64 `run` of `inputs(...)`, computed once and shared."""
    return run(inputs(P, B, T, C, K, variant), torch.float64, bias)


# ---------------------------------------------------------------------------------------
# the GPU matrix: (kernel class, what the row is there for, (P, B, T, C, K)).
# tests/test_convmod_core_gpu.py's docstring says how each class follows from the launcher.

CASES = [
    ("tiles48", "3groups-last6-3passes", (3, 2, 70, 144, 31)),
    ("tiles48", "1group-3tiles-last1", (1, 2, 129, 48, 31)),
    ("tiles32", "2groups-T64", (2, 2, 64, 64, 31)),
    ("tiles16", "5groups-T65", (3, 1, 65, 80, 31)),
    ("tiles16", "last8", (1, 1, 72, 16, 31)),
    ("tiles48", "T1", (1, 64, 1, 48, 31)),
    ("tiles48", "T8", (1, 8, 8, 48, 31)),
    ("tiles48", "T15", (1, 8, 15, 48, 31)),
    ("tiles48", "T16", (1, 4, 16, 48, 31)),
    ("row31-vec", "C36-3passes", (3, 1, 70, 36, 31)),
    ("row31-scalar", "C37", (1, 2, 70, 37, 31)),
    ("row31-scalar", "C37-3passes", (3, 1, 70, 37, 31)),
    ("row31-scalar", "C1", (1, 3, 33, 1, 31)),
    ("row31-vec", "TT32", (1, 2, 70, 256, 31)),
    ("row31-vec", "TT16-1024threads", (1, 1, 70, 320, 31)),
    ("generic", "K1", (1, 2, 50, 48, 1)),
    ("generic", "K3", (1, 2, 70, 48, 3)),
    ("generic", "K33", (1, 2, 100, 48, 33)),
    ("generic", "K127", (1, 1, 200, 16, 127)),
    ("generic", "K63-TT32", (1, 1, 70, 144, 63)),
    ("row31-scalar", "512chunks", (1, 1, 8200, 5, 31)),
    ("generic", "C1024-1lane-rowschunks-clamped", (1, 1, 130, 1024, 3)),
]
ONE_ROW = [("tiles48", "one-row-per-pass", (3, 1, 1, 48, 31)),
           ("row31-vec", "one-row-per-pass", (3, 1, 1, 36, 31))]
CASE_IDS = [f"{cls}-{name}" for cls, name, _ in CASES]
# the rows every variant runs on: the first tiles row and the row-vector whole-row one
def case(name):
    return next(c for c in CASES if c[1] == name)


VARIANT_ROWS = [CASES[0], case("C36-3passes")]

# The project's bars (tests/test_layernorm_family_gpu.py, tests/test_convmod_gpu.py).
REL_MAX, ABS_FLOOR = 1e-5, 1e-6   # v, z, g, du: max|err| <= REL_MAX * max|ref| + ABS_FLOOR
REL_L2 = 1e-5                     # dw_dw, dgamma, dbeta
STAT_REF = 1e-5                   # mean: * max|z|; rstd: relative -- against the reference
STAT_OWN = 1e-6                   # the same against float64 statistics of the device's own z
ZERO_ABS = 1e-5                   # db_dw (and dw_dw at K = 1): * max_c sum|terms|


def errors(got, ref):
    """{quantity: (err, bar)} of a run `got` (any dtype; a dict as `run` returns, dz not
    needed) against the float64 run `ref`, in the forms of the bars above."""
    d = lambda k: got[k].detach().double().cpu()  # noqa: E731
    out = {}
    for k in ("v", "z", "g", "du"):
        out[k] = ((d(k) - ref[k]).abs().max().item(), REL_MAX * ref[k].abs().max().item() + ABS_FLOOR)
    K = ref["dw_dw"].shape[-1]
    C = ref["z"].shape[1]
    for k in ("dw_dw", "dgamma", "dbeta"):
        if k == "dw_dw" and K == 1:
            continue
        n = ref[k].norm().item()
        if n == 0.0:  # an all-zero reference (one row per pass): the caller asserts exact zeros
            continue
        out[k] = (((d(k) - ref[k]).norm() / n).item(), REL_L2)
    zmax = ref["z"].abs().max().item()
    out["mean"] = ((d("mean").view(-1, C) - ref["mean"]).abs().max().item(), STAT_REF * zmax)
    out["rstd"] = (((d("rstd").view(-1, C) - ref["rstd"]).abs() / ref["rstd"]).max().item(), STAT_REF)
    # true zeros: bounded against the size of the terms that cancel
    if got.get("db_dw") is not None:
        out["db_dw"] = (d("db_dw").abs().max().item(),
                        ZERO_ABS * ref["dz"].abs().sum(dim=0).max().item())
    if K == 1:
        terms = (ref["dz"] * ref["g"]).abs().sum(dim=0).max().item()
        out["dw_dw"] = (d("dw_dw").abs().max().item(), ZERO_ABS * terms)
    return out
