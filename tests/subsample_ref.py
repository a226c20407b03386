"""Reference for Conv2dSubsampling's two convolutions (csrc/subsample.hip): no GPU code in here.

Written from the contract in include/onebit_hip.h ("Conv2dSubsampling's two convolutions") and
the layout comment at the top of csrc/subsample.hip, channels last:

    X  [B][T][F];  W0 [C][1][3][3], b0 [C];  W2 [C][C][3][3], b2 [C]
    pre1[b, t1, f1, c]  = sum_ij X[b, 2 t1 + i, 2 f1 + j] * W0[c, 0, i, j] + b0[c]
    Y1 = pre1 * m1,  m1 = pre1 > 0            T1 = (T - 3) // 2 + 1,  F1 = (F - 3) // 2 + 1
    pre2[b, t2, f2, o]  = sum_ij sum_c Y1[b, 2 t2 + i, 2 f2 + j, c] * W2[o, c, i, j] + b2[o]
    Y2 = pre2 * m2,  m2 = pre2 > 0            T2 = (T1 - 3) // 2 + 1, F2 = (F1 - 3) // 2 + 1
and for dY2 = dL/dY2:
    G = dY2 * m2;  db2 = sum G;  dW2[o, c, i, j] = sum G[b, t2, f2, o] * Y1[b, 2 t2 + i, 2 f2 + j, c]
    dY1[b, 2 t2 + i, 2 f2 + j, c] += sum_o G[b, t2, f2, o] * W2[o, c, i, j]
    D = dY1 * m1;  db0 = sum D;  dW0[c, 0, i, j] = sum D[b, t1, f1, c] * X[b, 2 t1 + i, 2 f1 + j]

Plain torch on CPU tensors: nine strided slices and an einsum per convolution, the backward
written out (no autograd, no F.conv2d; tests/test_subsample_ref_cpu.py checks it against both).
The masks can be given: a ReLU tie that float32 and float64 decide differently moves a gradient
by one whole term, which is no arithmetic error of either, so a comparison of gradients pins
them. `forward` / `backward` work in the dtype asked for: float64 is the reference, float32 measures what the
number format alone costs.

`plan` restates the host launch arithmetic of csrc/subsample.hip, so that every row of the
GPU matrix (the tables at the end, shared by the CPU and the GPU test) can assert the launch
property it is there for.
"""
from __future__ import annotations

import functools
import math

import torch

TAPS = [(i, j) for i in range(3) for j in range(3)]


def out_len(n):
    return (n - 3) // 2 + 1


def dims(T, F):
    T1, F1 = out_len(T), out_len(F)
    return T1, F1, out_len(T1), out_len(F1)


def _win(a, i, j, n_t, n_f):
    """a[:, 2 t + i, 2 f + j] for t < n_t, f < n_f: the tap (i, j) operand of a stride-2 conv."""
    return a[:, i:i + 2 * n_t - 1:2, j:j + 2 * n_f - 1:2]


def _conv0(x, w0, b0, T1, F1):
    pre = b0.expand(x.shape[0], T1, F1, -1).clone()
    for i, j in TAPS:
        pre += _win(x, i, j, T1, F1)[..., None] * w0[:, 0, i, j]
    return pre


def _conv2(y1, w2, b2, T2, F2):
    pre = b2.expand(y1.shape[0], T2, F2, -1).clone()
    for i, j in TAPS:
        pre += torch.einsum("btfc,oc->btfo", _win(y1, i, j, T2, F2), w2[:, :, i, j])
    return pre


def _back2(g, y1, w2):
    """dW2, db2, dY1 of pre2 = conv2(y1) for dL/dpre2 = g."""
    T2, F2 = g.shape[1:3]
    dw2 = torch.zeros_like(w2)
    dy1 = torch.zeros_like(y1)
    for i, j in TAPS:
        dw2[:, :, i, j] = torch.einsum("btfo,btfc->oc", g, _win(y1, i, j, T2, F2))
        _win(dy1, i, j, T2, F2).add_(torch.einsum("btfo,oc->btfc", g, w2[:, :, i, j]))
    return dw2, g.sum(dim=(0, 1, 2)), dy1


def _back0(d, x, w0):
    """dW0, db0 of pre1 = conv0(x) for dL/dpre1 = d."""
    T1, F1 = d.shape[1:3]
    dw0 = torch.zeros_like(w0)
    for i, j in TAPS:
        dw0[:, 0, i, j] = torch.einsum("btfc,btf->c", d, _win(x, i, j, T1, F1))
    return dw0, d.sum(dim=(0, 1, 2))


def forward(t, dtype=torch.float64, m1=None, m2=None):
    """pre1, Y1, pre2, Y2 of the inputs `t` (see `inputs`) in `dtype`, and the masks used: m1 / m2,
    boolean [B, T1, F1, C] / [B, T2, F2, C], replace pre1 > 0 / pre2 > 0 when given."""
    x, w0, b0, w2, b2 = (t[k].to(dtype) for k in ("x", "w0", "b0", "w2", "b2"))
    T1, F1, T2, F2 = dims(*x.shape[1:])
    pre1 = _conv0(x, w0, b0, T1, F1)
    m1 = pre1 > 0 if m1 is None else m1
    y1 = pre1 * m1
    pre2 = _conv2(y1, w2, b2, T2, F2)
    m2 = pre2 > 0 if m2 is None else m2
    return {"pre1": pre1, "Y1": y1, "pre2": pre2, "Y2": pre2 * m2, "m1": m1, "m2": m2}


def backward(t, f, m1=None, m2=None, abs_sums=False):
    """dW0, db0, dW2, db2 and dY1 (dL/dY1, before m1) for dL/dY2 = t["dy2"], from the forward
    `f` in its dtype. m1 / m2 default to the forward's; when given they replace them here too
    (Y1 = pre1 * m1). abs_sums: also "abs", the largest sum of absolute terms of every quantity,
    the forward's included (each input of a later sum bounded by its own sum of absolute terms),
    for inputs that are meant to be summed exactly."""
    dtype = f["pre1"].dtype
    x, w0, b0, w2, b2, dy2 = (t[k].to(dtype) for k in ("x", "w0", "b0", "w2", "b2", "dy2"))
    m1 = f["m1"] if m1 is None else m1
    m2 = f["m2"] if m2 is None else m2
    y1 = f["pre1"] * m1
    g = dy2 * m2
    dw2, db2, dy1 = _back2(g, y1, w2)
    dw0, db0 = _back0(dy1 * m1, x, w0)
    out = {"dY1": dy1, "dW0": dw0, "db0": db0, "dW2": dw2, "db2": db2}
    if abs_sums:
        T1, F1, T2, F2 = dims(*x.shape[1:])
        a_pre1 = _conv0(x.abs(), w0.abs(), b0.abs(), T1, F1)
        a_pre2 = _conv2(a_pre1 * m1, w2.abs(), b2.abs(), T2, F2)
        a_dw2, a_db2, a_dy1 = _back2(g.abs(), a_pre1 * m1, w2.abs())
        a_dw0, a_db0 = _back0(a_dy1 * m1, x.abs(), w0.abs())
        out["abs"] = {k: v.max().item() for k, v in
                      (("pre1", a_pre1), ("pre2", a_pre2), ("dW2", a_dw2), ("db2", a_db2),
                       ("dY1", a_dy1), ("dW0", a_dw0), ("db0", a_db0))}
    return out


def run(t, dtype=torch.float64, m1=None, m2=None, abs_sums=False):
    """`forward` and `backward` in one dict."""
    f = forward(t, dtype, m1, m2)
    f.update(backward(t, f, abs_sums=abs_sums))
    return f


# ---------------------------------------------------------------------------------------
# inputs


@functools.lru_cache(maxsize=8)
def inputs(B, T, F, C, kind="std"):
    """float32 CPU inputs, seeded on the CPU, shared and never modified.
    "std": X, dY2 ~ N(0, 1); weights ~ N(0, 1 / fan-in), biases ~ 0.1 N(0, 1).
    "int": X, b0, dY2 in {-2..2}, W0 in {-1, 0, 1}, W2 in {-1, 0, 1} with a tenth of it non-zero,
    b2 in {-3..3}: every product and (asserted by the tests) every sum an integer below 2^24,
    so float32 in any order, the three-way bf16 split included, is exact."""
    gen = torch.Generator().manual_seed(1000003 * C + 10007 * T + 101 * F + B)
    _, _, T2, F2 = dims(T, F)
    if kind == "int":
        def ri(lo, hi, *shape):
            return torch.randint(lo, hi + 1, shape, generator=gen).float()

        x, w0, b0 = ri(-2, 2, B, T, F), ri(-1, 1, C, 1, 3, 3), ri(-2, 2, C)
        w2 = (2 * ri(0, 1, C, C, 3, 3) - 1) * (torch.rand(C, C, 3, 3, generator=gen) < 0.1)
        b2, dy2 = ri(-3, 3, C), ri(-2, 2, B, T2, F2, C)
    else:
        assert kind == "std", kind
        rn = lambda *shape: torch.randn(*shape, generator=gen)  # noqa: E731
        x, w0, b0 = rn(B, T, F), rn(C, 1, 3, 3) / 3, rn(C) * 0.1
        w2, b2, dy2 = rn(C, C, 3, 3) / (9 * C) ** 0.5, rn(C) * 0.1, rn(B, T2, F2, C)
    return {"x": x, "w0": w0, "b0": b0, "w2": w2, "b2": b2, "dy2": dy2}


# ---------------------------------------------------------------------------------------
# bars: the project's (tests/test_subsample_gpu.py, tests/test_convmod_core_gpu.py), the
# gradients now per element as well. tests/test_subsample_ref_cpu.py shows that float32 alone,
# masks pinned, stays below half of each at every row of the matrix.

REL_MAX, ABS_FLOOR = 1e-5, 1e-6   # Y1, Y2: max|err| <= REL_MAX * max|ref| + ABS_FLOOR
REL_L2 = 1e-5                     # dW0, db0, dW2, db2: rel-L2
GRAD_MAX = 1e-5                   # ... and max|err| <= GRAD_MAX * max|ref|
FWD = ("Y1", "Y2")
GRADS = ("dW0", "db0", "dW2", "db2")


def fwd_bar(ref_y):
    return REL_MAX * ref_y.abs().max().item() + ABS_FLOOR


def errors(got, ref, keys=FWD + GRADS):
    """{quantity: (err, bar)} of `got` (any dtype) against the float64 `ref`. A gradient whose
    reference is all zeros is left out: the caller asserts exact zeros."""
    out = {}
    for k in keys:
        d = got[k].detach().double().cpu() - ref[k]
        if k in FWD:
            out[k] = (d.abs().max().item(), fwd_bar(ref[k]))
            continue
        n = ref[k].norm().item()
        if n == 0.0:
            continue
        out[k + "/l2"] = (d.norm().item() / n, REL_L2)
        out[k + "/max"] = (d.abs().max().item(), GRAD_MAX * ref[k].abs().max().item())
    return out


# ---------------------------------------------------------------------------------------
# the host launch arithmetic of csrc/subsample.hip, restated (line numbers of that file)

K_THR = 256            # kThr, :35
BM = 128               # GemmCfg::BM = 16 * WV * MR with WV = 4 (:192), MR = 2 (:854)
FWD_BLOCKS = 512       # launch_subsample_fwd's grid cap, :889
CONV0_BLOCKS = 8192    # launch_subsample_fwd's conv0 cap, :875
DGRAD_BLOCKS = 508     # kDgradBlocks, :800
DGRAD_EPI = 4          # kDgradEpi, :801
WG_BLOCKS = 256        # wg_plan's `want = 256 / tiles`, :822
WG_STEP = 32           # rows per wgrad step, :531 and :824
FINISH_IN_FLIGHT = 16  # ss_wgrad_finish_kernel's Gn, :713
WG_TILE = {144: (3, 3), 96: (3, 2), 48: (3, 1), 64: (2, 2)}  # (TW, WN = WK), wg_plan :813-817


def _ceil(a, b):
    return -(-a // b)


def _split(tiles, nblk):
    """Tiles of each block under t_begin = tiles * L / nblk, t_end = tiles * (L + 1) / nblk (:225)."""
    return [tiles * (L + 1) // nblk - tiles * L // nblk for L in range(nblk)]


def class_taps(cl):
    return (1 if cl >> 1 else 2) * (1 if cl & 1 else 2)  # :45-47


def plan(B, T, F, C):
    """What launch_subsample_fwd / launch_subsample_bwd do with a shape, as plain numbers."""
    T1, F1, T2, F2 = dims(T, F)
    M = B * T2 * F2
    p = {"T1": T1, "F1": F1, "T2": T2, "F2": F2, "M": M,
         # rows / columns that no window reads: (X rows, Y1 rows, X columns, Y1 columns), 0 or 1
         "unused": (T - (2 * T1 + 1), T1 - (2 * T2 + 1), F - (2 * F1 + 1), F1 - (2 * F2 + 1))}
    # conv0 (:873-877): ppb positions per block step, grid-stride over min(blocks, 8192)
    pos, ppb = B * T1 * F1, K_THR // (C // 4)
    blocks = min(_ceil(pos, ppb), CONV0_BLOCKS)
    p["conv0"] = {"positions": pos, "cap": CONV0_BLOCKS * ppb, "blocks": blocks,
                  "passes": _ceil(pos, blocks * ppb)}
    # forward GEMM (:887-890)
    tiles = _ceil(M, BM)
    nblk = min(tiles, FWD_BLOCKS)
    per = _split(tiles, nblk)
    p["fwd"] = {"tiles": tiles, "blocks": nblk, "tiles_per_block": (min(per), max(per)),
                "last_tile_rows": M - (tiles - 1) * BM}
    # dgrad classes (:935-953)
    cls, cost = [], []
    for cl in range(4):
        pt, pf = cl >> 1, cl & 1
        rows = B * (T1 // 2 if pt else (T1 + 1) // 2) * (F1 // 2 if pf else (F1 + 1) // 2)
        tl = _ceil(rows, BM)
        ks = _ceil(class_taps(cl) * C, 32)
        cls.append({"rows": rows, "tiles": tl, "ksteps": ks})
        cost.append(float(tl) * (ks + DGRAD_EPI))
    total = sum(cost)
    for c, k in zip(cls, cost):
        c["nblk"] = max(1, int(DGRAD_BLOCKS * k / total))
        per = _split(c["tiles"], c["nblk"])
        c["tiles_per_block"] = (min(per), max(per))
        c["empty_blocks"] = sum(1 for n in per if n == 0)
    p["dgrad"] = cls
    p["dgrad_blocks"] = sum(c["nblk"] for c in cls)
    # wgrad (:811-826)
    tw, wn = WG_TILE[C]
    wtiles = (C // (16 * tw * wn)) ** 2 * 9
    want = max(1, WG_BLOCKS // wtiles)
    rpc = WG_STEP * _ceil(M, want * WG_STEP)
    chunks = _ceil(M, rpc)
    last = M - (chunks - 1) * rpc
    p["wgrad"] = {"tiles": wtiles, "rows_per_chunk": rpc, "chunks": chunks,
                  "steps_first": _ceil(min(rpc, M), WG_STEP), "last_chunk_rows": last,
                  "steps_last": _ceil(last, WG_STEP)}
    return p


# ---------------------------------------------------------------------------------------
# the GPU matrix: (class, what the row is there for, (B, T, F, C)). The docstring of
# tests/test_subsample_family_gpu.py says how each follows from the launchers; `check_plan`
# asserts it.

CS = (48, 64, 96, 144)
SHIPPED = (16, 1000, 80)

CASES = (
    [("small", f"ragged-C{C}", (3, 39, 83, C)) for C in CS]
    + [("small", f"parity-T{T}-F{F}", (2, T, F, 48)) for T in (7, 8, 9, 10) for F in (7, 8, 9, 10)]
    + [("small", f"parity-T{T}-F80", (2, T, 80, 144)) for T in (35, 36, 37, 38)]
    + [("rows", f"M1-C{C}", (1, 7, 7, C)) for C in CS]
    + [("rows", "M128", (2, 35, 35, 64)),
       ("rows", "M129", (3, 175, 7, 96)),
       ("rows", "M140-last12", (4, 23, 31, 144)),
       ("wgrad", "1chunk-M22", (1, 11, 47, 48)),
       ("wgrad", "M896-28chunks", (4, 59, 67, 64)),
       ("wgrad", "M897-15chunks-last1", (3, 55, 95, 48)),
       ("wgrad", "M897-15chunks-last1-C144", (3, 55, 95, 144)),
       ("wgrad", "M1024-16chunks", (4, 67, 67, 64)),
       ("wgrad", "M1050-17chunks", (3, 59, 103, 48)),
       ("wgrad", "3steps", (5, 83, 83, 64)),
       ("wgrad", "4steps", (6, 83, 103, 48)),
       ("wgrad", "5steps", (4, 167, 103, 64)),
       ("wgrad", "5steps-C144", (4, 167, 103, 144))]
    + [("shipped", f"C{C}", SHIPPED + (C,)) for C in CS]
)
CASE_IDS = [f"{cls}-{name}" for cls, name, _ in CASES]
INT_CASES = [(3, 23, 31, 48), (2, 25, 33, 144)]


def case(name):
    return next(c for c in CASES if c[1] == name)


def check_plan(cls, name, shape):
    """Assert, through `plan`, the launch property the row (cls, name, shape) is there for."""
    p = plan(*shape)
    B, T, F, C = shape
    fw, wg, dg = p["fwd"], p["wgrad"], p["dgrad"]
    if name.startswith("ragged"):
        # odd T1 and F1: the four dgrad classes all differ in size; ragged last tile
        assert p["T1"] % 2 == 1 and p["F1"] % 2 == 1
        assert len({c["rows"] for c in dg}) == 4 and p["M"] % BM not in (0, 1)
    elif name.startswith("parity"):
        # T % 4, F % 4 decide whether X's and Y1's last row / column are read at all; the CPU
        # test asserts that the rows together take every combination
        u = p["unused"]
        assert u[0] == (T + 1) % 2 and u[2] == (F + 1) % 2 and set(u) <= {0, 1}
        assert u[1] == (1 if T % 4 in (1, 2) else 0) and u[3] == (1 if F % 4 in (1, 2) else 0)
        assert C != 48 or p["M"] == 2
    elif name.startswith("M1-"):
        assert p["M"] == 1 and [c["rows"] for c in dg] == [4, 2, 2, 1]
        assert sum(c["empty_blocks"] for c in dg) == p["dgrad_blocks"] - 4 >= 500
        assert wg["chunks"] == 1 and wg["steps_first"] == 1
    elif name == "M128":
        assert p["M"] == BM and fw["tiles"] == 1 and fw["last_tile_rows"] == BM
    elif name == "M129":
        assert p["M"] == BM + 1 and fw["tiles"] == 2 and fw["last_tile_rows"] == 1
    elif name == "M140-last12":
        assert fw["tiles"] == 2 and 1 < fw["last_tile_rows"] <= 16
    elif name == "1chunk-M22":
        assert 1 < p["M"] < WG_STEP and wg["chunks"] == 1 and wg["steps_first"] == 1
    elif name == "M896-28chunks":
        assert p["M"] == 896 and wg["chunks"] == 28 and wg["rows_per_chunk"] == WG_STEP
        assert wg["steps_first"] == wg["steps_last"] == 1
    elif name.startswith("M897"):
        assert p["M"] == 897 and wg["chunks"] == FINISH_IN_FLIGHT - 1 and wg["last_chunk_rows"] == 1
        assert wg["steps_first"] == 2
    elif name == "M1024-16chunks":
        assert p["M"] == 1024 and wg["chunks"] == FINISH_IN_FLIGHT and wg["last_chunk_rows"] == 64
    elif name == "M1050-17chunks":
        assert 1025 <= p["M"] <= 1088 and wg["chunks"] == FINISH_IN_FLIGHT + 1
    elif name[0] in "345" and "steps" in name:
        assert wg["steps_first"] == int(name[0]) and wg["chunks"] > FINISH_IN_FLIGHT
    else:
        assert cls == "shipped", (cls, name)
        assert fw["tiles"] == 592 > FWD_BLOCKS == fw["blocks"] and fw["tiles_per_block"] == (1, 2)
        for c in dg:  # every class: more tiles than blocks, and no block without a tile
            assert c["tiles"] > c["nblk"] and c["tiles_per_block"][0] >= 2 and c["empty_blocks"] == 0
        assert p["conv0"]["positions"] > p["conv0"]["cap"] and p["conv0"]["passes"] >= 2
        assert wg["steps_first"] >= 64 and wg["chunks"] == 28
    if cls == "wgrad":
        assert wg["tiles"] == 9 and wg["rows_per_chunk"] == WG_STEP * math.ceil(p["M"] / 896)
    return p
