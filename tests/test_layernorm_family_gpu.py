"""Every entry point of csrc/layernorm.hip, at every column-slot class, against float64.

The launcher compiles each kernel for nine column-slot classes: the vector path (d % 4 == 0,
every operand 16-byte aligned) by ceil(d / 64) in {1, 2, 3, 4, 8}, the scalar path by
ceil(d / 16) in {4, 9, 16, 32}. The matrix below has one d at each class edge, plus
d % 4 == 0 shapes whose operands start one float into a larger buffer (scalar fallback).
References are tests/layernorm_ref.py: float64 torch on the CPU, and the restated keep-hash
(never the device's own mask). The kernels' inputs (statistics, y1) are float32 casts of the
float64 reference, so no check leans on another kernel's output.

Bars (tests/test_layernorm_gpu.py's): y, dx, dy2 max|err| <= 1e-5 * max|ref| + 1e-6;
dgamma, dbeta rel-L2 <= 1e-5; mean max|err| <= 1e-6 * max|x|; rstd rel <= 1e-6.
"""
import functools

import numpy as np
import pytest
import torch

import layernorm_ref as R

pytestmark = pytest.mark.gpu

OB_OK, OB_ERR_NULL, OB_ERR_SHAPE, OB_ERR_WORKSPACE, OB_ERR_ALIGN = 0, -1, -2, -4, -5

D_VEC = [4, 64, 68, 128, 132, 192, 196, 256, 260, 512]
D_SCAL = [1, 63, 65, 143, 145, 255, 257, 511]
D_MIS = [64, 144, 256, 512]
MATRIX = [(d, 0) for d in D_VEC + D_SCAL] + [(d, 1) for d in D_MIS]
_IDS = [f"d{d}{'-misaligned' if off else ''}" for d, off in MATRIX]
ROWS = 37  # two full 16-row blocks and a 5-row tail
EPS, EPS2 = 1e-5, 1e-3
SEED, CTR, RNG_OFF = 2**40 + 3, 2**33 + 1, 9  # the GradScale dropout stream
P_DROP, RSCALE = 0.1, 0.5

_WORST = {}  # (entry, quantity) -> (err / bar, err, bar, where)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if _WORST:
        print("\nworst observed error per entry point (err, bar, where):")
        for (entry, q), (_, err, bar, where) in sorted(_WORST.items()):
            print(f"  {entry:10s} {q:7s} {err:.3e}  bar {bar:.3e}  {where}")


@pytest.fixture(scope="module")
def lib(gpu):
    from onebit_asr import _lib

    return _lib.load()


# ---------------------------------------------------------------------------------------
# comparisons: every message carries the observed error and its bar


def _note(entry, q, err, bar, where):
    ratio = err / bar if bar > 0 else 0.0
    if (entry, q) not in _WORST or ratio > _WORST[(entry, q)][0]:
        _WORST[(entry, q)] = (ratio, err, bar, where)


def _cpu(t):
    return t.detach().cpu().double()


def close(entry, q, a, ref, where, floor=0.0):
    """max|a - ref| <= max(1e-5 * max|ref| + 1e-6, floor)"""
    a, ref = _cpu(a), ref.double()
    assert a.shape == ref.shape, (entry, q, a.shape, ref.shape)
    if a.numel() == 0:
        return
    assert torch.isfinite(a).all(), f"{entry} {q} {where}: non-finite output"
    err = (a - ref).abs().max().item()
    bar = max(1e-5 * ref.abs().max().item() + 1e-6, floor)
    _note(entry, q, err, bar, where)
    assert err <= bar, f"{entry} {q} {where}: max|err| {err:.3e} > bar {bar:.3e}"


def rel_l2(entry, q, a, ref, where, floor=0.0, zero=False):
    """|a - ref|_2 / |ref|_2 <= max(1e-5, floor); zero (dgamma at d = 1: xhat is exactly 0 in
    the reference and in the kernel's arithmetic) or an all-zero reference: exact zeros"""
    a, ref = _cpu(a), ref.double()
    assert torch.isfinite(a).all(), f"{entry} {q} {where}: non-finite output"
    if zero or ref.norm().item() == 0.0:
        assert ref.abs().max().item() <= 1e-12, f"{entry} {q} {where}: reference not zero"
        assert (a == 0).all(), f"{entry} {q} {where}: expected exact zeros, max|a| {a.abs().max().item():.3e}"
        return
    err = ((a - ref).norm() / ref.norm()).item()
    bar = max(1e-5, floor)
    _note(entry, q, err, bar, where)
    assert err <= bar, f"{entry} {q} {where}: rel-L2 {err:.3e} > bar {bar:.3e}"


def mean_close(entry, q, a, ref, xmax, where, floor=0.0):
    a = _cpu(a)
    if a.numel() == 0:
        return
    err = (a - ref).abs().max().item()
    bar = max(1e-6 * xmax, floor)
    _note(entry, q, err, bar, where)
    assert err <= bar, f"{entry} {q} {where}: max|err| {err:.3e} > bar {bar:.3e}"


def rstd_close(entry, q, a, ref, where, floor=0.0):
    a = _cpu(a)
    if a.numel() == 0:
        return
    err = ((a - ref).abs() / ref.abs()).max().item()
    bar = max(1e-6, floor)
    _note(entry, q, err, bar, where)
    assert err <= bar, f"{entry} {q} {where}: max rel err {err:.3e} > bar {bar:.3e}"


def bitwise(a, b, what):
    a, b = a.detach().cpu(), b.detach().cpu()
    same = torch.equal(a, b)
    assert same, f"{what}: {int((a != b).sum())} of {a.numel()} elements differ"


# ---------------------------------------------------------------------------------------
# inputs (CPU-seeded, shared, never modified) and their float64 references


@functools.lru_cache(maxsize=None)
def inputs(rows, d, kind="std"):
    g = torch.Generator().manual_seed(1000 * d + rows)
    x = torch.randn(rows, d, generator=g)
    if kind in ("std", "zeros"):
        x = x * 3 + 1
    elif kind == "small":
        x = x * 1e-3
    elif kind == "off30":
        x = x + 30
    if kind == "zeros":  # padded frames: all-zero rows in the first block, mid-block, the tail
        x[[r for r in (0, 5, 16, 31, rows - 1) if r < rows]] = 0.0
    t = {"x": x, "g": torch.randn(d, generator=g) * 0.5 + 1, "b": torch.randn(d, generator=g),
         "dy": torch.randn(rows, d, generator=g), "dres": torch.randn(rows, d, generator=g),
         "g2": torch.randn(d, generator=g) * 0.5 + 1, "b2": torch.randn(d, generator=g)}
    return t


@functools.lru_cache(maxsize=None)
def ref_fwd(rows, d, kind="std", gamma=True, beta=True):
    t = inputs(rows, d, kind)
    return R.ln_fwd(t["x"], t["g"] if gamma else None, t["b"] if beta else None, EPS)


@functools.lru_cache(maxsize=None)
def ref_bwd(rows, d, kind="std", gamma=True):
    t = inputs(rows, d, kind)
    return R.ln_bwd(t["x"], t["g"] if gamma else None, EPS, t["dy"])


@functools.lru_cache(maxsize=None)
def ref_pair_fwd(rows, d, g1=True, g2=True):
    t = inputs(rows, d)
    return R.ln_pair_fwd(t["x"], t["g"] if g1 else None, t["b"], EPS,
                         t["g2"] if g2 else None, t["b2"], EPS2)


@functools.lru_cache(maxsize=None)
def ref_pair_bwd(rows, d, gres, g1=True, g2=True):
    t = inputs(rows, d)
    return R.ln_pair_bwd(t["x"], t["g"] if g1 else None, t["b"], EPS, t["g2"] if g2 else None,
                         EPS2, t["dy"], t["dres"] if gres else None)


def gs_layout(rows):
    """(T, lens) of the GradScale cases: T = 13 and lens = [T, T // 2, 0] at rows = 39; other
    row counts keep the pattern (full, half, empty utterances) as far as rows divide."""
    if rows % 13 == 0:
        T = 13
    elif rows % 3 == 0:
        T = rows // 3
    else:
        T = max(rows, 1)
    B = rows // T if rows else 0
    lens = ([T, T // 2, 0] * B)[:B] if B >= 3 else [T // 2] * B
    return T, lens


@functools.lru_cache(maxsize=None)
def keep_mask(rows, d):
    return R.np_keep_flat(SEED, CTR + RNG_OFF, rows * d, P_DROP).reshape(rows, d)


# ---------------------------------------------------------------------------------------
# device placement and the raw calls


def put(t, gpu, off=0):
    """CPU tensor -> device. off: a contiguous view starting one float (4 bytes) into a larger
    buffer, so its address is 4 mod 16 and the launcher must leave the vector path."""
    if t is None:
        return None
    t = t.contiguous()
    if not off:
        return t.to(gpu)
    nbytes = t.numel() * t.element_size()
    buf = torch.empty(nbytes + 32, dtype=torch.uint8, device=gpu)
    v = buf[4:4 + nbytes].view(t.dtype).view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def f32(t, gpu, off=0):
    return put(t.float(), gpu, off)


def nans(shape, gpu, off=0):
    return put(torch.full(tuple(shape) if not isinstance(shape, int) else (shape,), float("nan")), gpu, off)


def q_out(rows, d, gpu, off=0):
    return put(torch.full((rows, d), -128, dtype=torch.int8), gpu, off)  # -128 is never written


def P(t):
    return t if t is None or isinstance(t, int) else t.data_ptr()


def stream(gpu):
    return torch.cuda.current_stream(gpu).cuda_stream


def alloc_ws(nbytes, gpu):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=gpu)


def rng_tensor(gpu):
    # (never offset: the kernels read {seed, counter} as 64-bit words; nor are the workspaces,
    # ob_layernorm_bwd_pair requires its own 16-byte aligned)
    return torch.tensor([SEED, CTR], dtype=torch.int64, device=gpu)


def c_fwd(lib, gpu, x, g, b, rows, d, eps, y, mean, rstd):
    return lib.ob_layernorm_fwd(P(x), P(g), P(b), rows, d, eps, P(y), P(mean), P(rstd), stream(gpu))


def c_fwd_pair(lib, gpu, x, g1, b1, g2, b2, rows, d, e1, e2, y1, m1, r1, y2, m2, r2):
    return lib.ob_layernorm_fwd_pair(P(x), P(g1), P(b1), P(g2), P(b2), rows, d, e1, e2, P(y1), P(m1),
                                     P(r1), P(y2), P(m2), P(r2), stream(gpu))


def c_fwd_amax(lib, gpu, x, g, b, rows, d, eps, y, mean, rstd, Pn, amax, ws, wsb):
    return lib.ob_layernorm_fwd_amax(P(x), P(g), P(b), rows, d, eps, P(y), P(mean), P(rstd), Pn,
                                     P(amax), P(ws), wsb, stream(gpu))


def c_fwd_i8(lib, gpu, x, g, b, rows, d, eps, Pn, amax, yq, ws, wsb):
    return lib.ob_layernorm_fwd_i8(P(x), P(g), P(b), rows, d, eps, Pn, P(amax), P(yq), P(ws), wsb,
                                   stream(gpu))


def c_bwd(lib, gpu, dy, x, g, mean, rstd, rows, d, dx, dg, db, ws, wsb):
    return lib.ob_layernorm_bwd(P(dy), P(x), P(g), P(mean), P(rstd), rows, d, P(dx), P(dg), P(db),
                                P(ws), wsb, stream(gpu))


def c_bwd_res(lib, gpu, dy, x, g, mean, rstd, rows, d, dres, dx, dg, db, ws, wsb):
    return lib.ob_layernorm_bwd_res(P(dy), P(x), P(g), P(mean), P(rstd), rows, d, P(dres), P(dx),
                                    P(dg), P(db), P(ws), wsb, stream(gpu))


def c_bwd_ex(lib, gpu, dy, x, g, mean, rstd, rows, d, dres, dx, dg, db, ws, wsb, dy2, rscale, p,
             rng, off, lens, T):
    return lib.ob_layernorm_bwd_ex(P(dy), P(x), P(g), P(mean), P(rstd), rows, d, P(dres), P(dx),
                                   P(dg), P(db), P(ws), wsb, P(dy2), rscale, p, P(rng), off, P(lens),
                                   T, stream(gpu))


def c_bwd_defer(lib, gpu, dy, x, g, mean, rstd, rows, d, dres, dx, dg, db, ws, wsb, dy2, rscale, p,
                rng, off, lens, T, table, slot):
    return lib.ob_layernorm_bwd_defer(P(dy), P(x), P(g), P(mean), P(rstd), rows, d, P(dres), P(dx),
                                      P(dg), P(db), P(ws), wsb, P(dy2), rscale, p, P(rng), off,
                                      P(lens), T, P(table), slot, stream(gpu))


def c_bwd_pair(lib, gpu, dy, y1, g2, m2, r2, gres, x, g1, m1, r1, rows, d, dx, dg2, db2, dg1, db1,
               ws, wsb, dy2, rscale, p, rng, off, lens, T, table=None, s2=-1, s1=-1):
    return lib.ob_layernorm_bwd_pair(P(dy), P(y1), P(g2), P(m2), P(r2), P(gres), P(x), P(g1), P(m1),
                                     P(r1), rows, d, P(dx), P(dg2), P(db2), P(dg1), P(db1), P(ws),
                                     wsb, P(dy2), rscale, p, P(rng), off, P(lens), T, P(table), s2,
                                     s1, stream(gpu))


def np_quant(y: np.ndarray, amax) -> np.ndarray:
    """clip(rint(y * (127 / max(amax, 1e-5))), +-127) in fp32, as test_i8_fused_gpu._np_quant"""
    gam = np.float32(max(np.float32(amax), np.float32(1e-5)))
    sx = np.float32(np.float32(127.0) / gam)
    return np.clip(np.rint((y.astype(np.float32) * sx).astype(np.float32)), -127, 127).astype(np.int8)


# ---------------------------------------------------------------------------------------
# one check per entry point, used by the d x alignment matrix and by the row-count edges


def check_fwd(lib, gpu, rows, d, off, kind="std", floors=None):
    """ob_layernorm_fwd: y, mean, rstd against float64 (also gamma / beta NULL). Returns y."""
    t = inputs(rows, d, kind)
    where = f"rows {rows} d {d} off {off} {kind}"
    fl = floors or {}
    ent = "fwd" if kind == "std" else f"fwd/{kind}"
    x, g, b = (f32(t[k], gpu, off) for k in ("x", "g", "b"))
    xmax = t["x"].abs().max().item() if rows else 0.0
    y_full = None
    for use_g, use_b in ((True, True), (False, True), (True, False), (False, False)):
        if (kind != "std" or rows != ROWS) and not (use_g and use_b):
            continue
        y, mean, rstd = nans((rows, d), gpu, off), nans(rows, gpu, off), nans(rows, gpu, off)
        st = c_fwd(lib, gpu, x, g if use_g else None, b if use_b else None, rows, d, EPS, y, mean, rstd)
        assert st == OB_OK, (where, st)
        yr, mr, rr = ref_fwd(rows, d, kind, use_g, use_b)
        w = f"{where} gamma {use_g} beta {use_b}"
        close(ent, "y", y, yr, w, fl.get("y", 0.0))
        mean_close(ent, "mean", mean, mr, xmax, w, fl.get("mean", 0.0))
        rstd_close(ent, "rstd", rstd, rr, w, fl.get("rstd", 0.0))
        if use_g and use_b:
            y_full = y
    return y_full


def check_fwd_pair(lib, gpu, rows, d, off):
    t = inputs(rows, d)
    where = f"rows {rows} d {d} off {off}"
    x, g1, b1, g2, b2 = (f32(t[k], gpu, off) for k in ("x", "g", "b", "g2", "b2"))
    o = [nans(s, gpu, off) for s in ((rows, d), rows, rows, (rows, d), rows, rows)]
    assert c_fwd_pair(lib, gpu, x, g1, b1, g2, b2, rows, d, EPS, EPS2, *o) == OB_OK, where
    ref = ref_pair_fwd(rows, d)
    xmax = t["x"].abs().max().item()
    close("fwd_pair", "y1", o[0], ref[0], where)
    mean_close("fwd_pair", "mean1", o[1], ref[1], xmax, where)
    rstd_close("fwd_pair", "rstd1", o[2], ref[2], where)
    close("fwd_pair", "y2", o[3], ref[3], where)
    mean_close("fwd_pair", "mean2", o[4], ref[4], ref[0].abs().max().item(), where)
    rstd_close("fwd_pair", "rstd2", o[5], ref[5], where)
    # ... and bit for bit two plain launches (the second on the first's y1)
    s = [nans(sh, gpu, off) for sh in ((rows, d), rows, rows, (rows, d), rows, rows)]
    assert c_fwd(lib, gpu, x, g1, b1, rows, d, EPS, s[0], s[1], s[2]) == OB_OK
    assert c_fwd(lib, gpu, s[0], g2, b2, rows, d, EPS2, s[3], s[4], s[5]) == OB_OK
    for a, b_, name in zip(o, s, ("y1", "mean1", "rstd1", "y2", "mean2", "rstd2")):
        bitwise(a, b_, f"fwd_pair {name} vs two ob_layernorm_fwd {where}")
    # g1 / g2 / b1 / b2 NULL once
    if rows == ROWS:
        o = [nans(sh, gpu, off) for sh in ((rows, d), rows, rows, (rows, d), rows, rows)]
        assert c_fwd_pair(lib, gpu, x, None, b1, None, b2, rows, d, EPS, EPS2, *o) == OB_OK
        ref = ref_pair_fwd(rows, d, False, False)
        close("fwd_pair", "y1", o[0], ref[0], where + " g1 g2 NULL")
        close("fwd_pair", "y2", o[3], ref[3], where + " g1 g2 NULL")


def check_amax_i8(lib, gpu, x_cpu, g_cpu, b_cpu, eps, Pn, off, where):
    """fwd_amax: y bitwise the plain forward's, amax[p] == max|y[pass p]| exactly; fwd_i8: the
    same amax, the int8 image == np_quant(y[pass p], amax[p]) element for element."""
    rows, d = x_cpu.shape
    x, g, b = f32(x_cpu, gpu, off), f32(g_cpu, gpu, off), (f32(b_cpu, gpu, off) if b_cpu is not None else None)
    y0, m0, r0 = nans((rows, d), gpu, off), nans(rows, gpu, off), nans(rows, gpu, off)
    assert c_fwd(lib, gpu, x, g, b, rows, d, eps, y0, m0, r0) == OB_OK, where
    wsb = lib.ob_layernorm_fwd_amax_workspace(Pn)
    assert wsb > 0
    ws = alloc_ws(wsb, gpu)
    y, mean, rstd, amax = nans((rows, d), gpu, off), nans(rows, gpu, off), nans(rows, gpu, off), nans(Pn, gpu, off)
    assert c_fwd_amax(lib, gpu, x, g, b, rows, d, eps, y, mean, rstd, Pn, amax, ws, wsb) == OB_OK, where
    bitwise(y, y0, f"fwd_amax y vs fwd {where}")
    bitwise(mean, m0, f"fwd_amax mean vs fwd {where}")
    bitwise(rstd, r0, f"fwd_amax rstd vs fwd {where}")
    yc = y0.cpu()
    want = yc.view(Pn, rows // Pn, d).abs().amax(dim=(1, 2))
    got = amax.cpu()
    assert torch.equal(got, want), f"fwd_amax {where}: amax {got.tolist()} != max|y| per pass {want.tolist()}"
    amax8, yq = nans(Pn, gpu, off), q_out(rows, d, gpu, off)
    ws.fill_(0xFF)
    assert c_fwd_i8(lib, gpu, x, g, b, rows, d, eps, Pn, amax8, yq, ws, wsb) == OB_OK, where
    got8 = amax8.cpu()
    assert torch.equal(got8, want), f"fwd_i8 {where}: amax {got8.tolist()} != {want.tolist()}"
    q = yq.cpu().numpy().reshape(Pn, rows // Pn, d)
    yn = yc.numpy().reshape(Pn, rows // Pn, d)
    for p in range(Pn):
        ref = np_quant(yn[p], want[p].item())
        bad = int((q[p] != ref).sum())
        assert bad == 0, f"fwd_i8 {where}: pass {p}: {bad} of {ref.size} int8 elements differ"
    return want


def _stats32(rows, d, kind, gpu, off, gamma=True):
    _, mr, rr = ref_fwd(rows, d, kind, gamma, True)
    return f32(mr, gpu, off), f32(rr, gpu, off)


def check_bwd(lib, gpu, rows, d, off, kind="std", floors=None, variants=True):
    """ob_layernorm_bwd: dx / dgamma / dbeta, the dgamma-only, dbeta-only, neither (ws NULL)
    and gamma NULL variants; every call twice, bitwise equal."""
    t = inputs(rows, d, kind)
    where = f"rows {rows} d {d} off {off} {kind}"
    fl = floors or {}
    ent = "bwd" if kind == "std" else f"bwd/{kind}"
    dy, x, g = (f32(t[k], gpu, off) for k in ("dy", "x", "g"))
    mean, rstd = _stats32(rows, d, kind, gpu, off)
    wsb = lib.ob_layernorm_bwd_workspace(rows, d)
    ws = alloc_ws(wsb, gpu)
    dxr, dgr, dbr = ref_bwd(rows, d, kind)
    cases = [(True, True, True), (True, False, True), (False, True, True), (False, False, True),
             (True, True, False)]
    for want_g, want_b, use_g in (cases if variants else cases[:1]):
        w = f"{where} dgamma {want_g} dbeta {want_b} gamma {use_g}"
        rx, rg, rb = (dxr, dgr, dbr) if use_g else ref_bwd(rows, d, kind, False)
        runs = []
        for _ in range(2):
            dx = nans((rows, d), gpu, off)
            dg = nans(d, gpu, off) if want_g else None
            db = nans(d, gpu, off) if want_b else None
            params = want_g or want_b
            st = c_bwd(lib, gpu, dy, x, g if use_g else None, mean, rstd, rows, d, dx, dg, db,
                       ws if params else None, wsb if params else 0)
            assert st == OB_OK, (w, st)
            runs.append((dx, dg, db))
        for a, b_ in zip(*runs):
            if a is not None:
                bitwise(a, b_, f"bwd run-to-run {w}")
        dx, dg, db = runs[0]
        if d == 1:  # exactly 0 in the reference and in the kernel's arithmetic
            assert (dx.cpu() == 0).all(), f"bwd dx {w}: expected exact zeros"
        close(ent, "dx", dx, rx, w, fl.get("dx", 0.0))
        if dg is not None:
            rel_l2(ent, "dgamma", dg, rg, w, fl.get("dgamma", 0.0), zero=d == 1)
        if db is not None:
            rel_l2(ent, "dbeta", db, rb, w, fl.get("dbeta", 0.0))


def _gs_cases(rows):
    T, lens = gs_layout(rows)
    return [("full", P_DROP, RSCALE, lens, T), ("lens-only", 0.0, RSCALE, lens, T),
            ("drop-only", P_DROP, 1.0, None, 0)]


def _check_dy2(entry, dy2, dx_ref, rows, d, p, rscale, lens, T, where):
    keep = keep_mask(rows, d) if p > 0 else None
    ref = R.grad_scale(dx_ref, rscale, p, keep, lens, T)
    close(entry, "dy2", dy2, ref, where)
    live = torch.ones(rows, d, dtype=torch.bool)
    if keep is not None:
        live &= torch.from_numpy(keep)
    if lens is not None:
        live &= R.row_valid(rows, T, lens)[:, None]
    got = dy2.cpu()
    assert (got[~live] == 0).all(), f"{entry} dy2 {where}: a dropped / padded element is not exactly 0"
    # (a kept element that came out 0 where the reference is above the bar fails `close`)


def check_bwd_res_ex(lib, gpu, rows, d, off):
    """ob_layernorm_bwd_res: dx == ref dx + dres; ob_layernorm_bwd_ex: its dx / dgamma / dbeta
    and dy2 against the GradScale reference built on the restated hash."""
    t = inputs(rows, d)
    where = f"rows {rows} d {d} off {off}"
    dy, x, g, dres = (f32(t[k], gpu, off) for k in ("dy", "x", "g", "dres"))
    mean, rstd = _stats32(rows, d, "std", gpu, off)
    wsb = lib.ob_layernorm_bwd_workspace(rows, d)
    ws = alloc_ws(wsb, gpu)
    dxr, dgr, dbr = ref_bwd(rows, d)
    dxres = dxr + t["dres"].double()
    runs = []
    for _ in range(2):
        dx, dg, db = nans((rows, d), gpu, off), nans(d, gpu, off), nans(d, gpu, off)
        assert c_bwd_res(lib, gpu, dy, x, g, mean, rstd, rows, d, dres, dx, dg, db, ws, wsb) == OB_OK
        runs.append((dx, dg, db))
    for a, b_ in zip(*runs):
        bitwise(a, b_, f"bwd_res run-to-run {where}")
    close("bwd_res", "dx", runs[0][0], dxres, where)
    rel_l2("bwd_res", "dgamma", runs[0][1], dgr, where, zero=d == 1)
    rel_l2("bwd_res", "dbeta", runs[0][2], dbr, where)
    rng = rng_tensor(gpu)
    for name, p, rscale, lens, T in _gs_cases(rows):
        w = f"{where} {name}"
        lens_d = put(torch.tensor(lens, dtype=torch.int32), gpu, off) if lens is not None else None
        use_res = name != "lens-only"  # dres NULL once
        runs = []
        for _ in range(2):
            dx, dg, db = nans((rows, d), gpu, off), nans(d, gpu, off), nans(d, gpu, off)
            dy2 = nans((rows, d), gpu, off)
            st = c_bwd_ex(lib, gpu, dy, x, g, mean, rstd, rows, d, dres if use_res else None, dx, dg,
                          db, ws, wsb, dy2, rscale, p, rng, RNG_OFF, lens_d, T)
            assert st == OB_OK, (w, st)
            runs.append((dx, dg, db, dy2))
        for a, b_ in zip(*runs):
            bitwise(a, b_, f"bwd_ex run-to-run {w}")
        dx, dg, db, dy2 = runs[0]
        rx = dxres if use_res else dxr
        close("bwd_ex", "dx", dx, rx, w)
        rel_l2("bwd_ex", "dgamma", dg, dgr, w, zero=d == 1)
        rel_l2("bwd_ex", "dbeta", db, dbr, w)
        _check_dy2("bwd_ex", dy2, rx, rows, d, p, rscale, lens, T, w)


def check_bwd_pair(lib, gpu, rows, d, off):
    """ob_layernorm_bwd_pair against float64 autograd through both LNs: with / without gres,
    with / without the GradScale output, g1 / g2 NULL once; every call twice."""
    t = inputs(rows, d)
    where = f"rows {rows} d {d} off {off}"
    dy, x, g1, g2, gres = (f32(t[k], gpu, off) for k in ("dy", "x", "g", "g2", "dres"))
    wsb = lib.ob_layernorm_bwd_pair_workspace(rows, d)
    ws = alloc_ws(wsb, gpu)  # (16-byte aligned by contract: not offset)
    rng = rng_tensor(gpu)
    T, lens = gs_layout(rows)
    lens_d = put(torch.tensor(lens, dtype=torch.int32), gpu, off)
    cases = [("gres", True, None, True), ("plain", False, None, True),
             ("gres+gscale", True, ("full", P_DROP, RSCALE, lens, T), True),
             ("gscale lens-only", False, ("lens-only", 0.0, RSCALE, lens, T), True),
             ("gscale drop-only", True, ("drop-only", P_DROP, 1.0, None, 0), True),
             ("g1 g2 NULL", True, None, False)]
    for name, use_res, gs, use_g in cases:
        w = f"{where} {name}"
        fw = ref_pair_fwd(rows, d, use_g, use_g)
        y1, m1, r1, m2, r2 = (f32(fw[i], gpu, off) for i in (0, 1, 2, 4, 5))
        runs = []
        for _ in range(2):
            dx = nans((rows, d), gpu, off)
            dg2, db2, dg1, db1 = (nans(d, gpu, off) for _ in range(4))
            dy2 = nans((rows, d), gpu, off) if gs else None
            _, p, rscale, ln, Tn = gs if gs else (None, 0.0, 1.0, None, 0)
            st = c_bwd_pair(lib, gpu, dy, y1, g2 if use_g else None, m2, r2, gres if use_res else None,
                            x, g1 if use_g else None, m1, r1, rows, d, dx, dg2, db2, dg1, db1, ws, wsb,
                            dy2, rscale, p, rng, RNG_OFF, lens_d if ln is not None else None, Tn)
            assert st == OB_OK, (w, st)
            runs.append((dx, dg1, db1, dg2, db2, dy2))
        for a, b_ in zip(*runs):
            if a is not None:
                bitwise(a, b_, f"bwd_pair run-to-run {w}")
        ref = ref_pair_bwd(rows, d, use_res, use_g, use_g)
        dx, dg1, db1, dg2, db2, dy2 = runs[0]
        if d == 1:
            assert (dx.cpu() == 0).all(), f"bwd_pair dx {w}: expected exact zeros"
        close("bwd_pair", "dx", dx, ref[0], w)
        for q, a, r in (("dg1", dg1, ref[1]), ("db1", db1, ref[2]), ("dg2", dg2, ref[3]),
                        ("db2", db2, ref[4])):
            # d = 1: xhat = 0 and LN2's dx = 0, so dg1, dg2 and (without gres) db1 are 0
            zero = d == 1 and (q in ("dg1", "dg2") or (q == "db1" and not use_res))
            rel_l2("bwd_pair", q, a, r, w, zero=zero)
        if gs:
            _check_dy2("bwd_pair", dy2, ref[0], rows, d, gs[1], gs[2], gs[3], gs[4], w)


# ---------------------------------------------------------------------------------------
# 2. the device hash == the restatement


@pytest.mark.parametrize("seed", [12345, 2**40 + 3])
@pytest.mark.parametrize("ctr", [7, 2**33 + 1])
def test_device_hash_is_the_restated_hash(gpu, lib, seed, ctr):
    rng = torch.tensor([seed, ctr], dtype=torch.int64, device=gpu)
    shapes = [(1, 1), (1, 2), (1, 1001), (7, 5), (6, 8)]  # (rows, row_len); rows 1 = flat
    for rows, T in shapes:
        n = rows * T
        for p in (0.0, 0.1, 0.5):
            for off in (0, 9):
                out = torch.full((n,), 7, dtype=torch.uint8, device=gpu)
                st = lib.ob_relattn_dropout_mask(n, T, p, rng.data_ptr(), off, out.data_ptr(),
                                                 stream(gpu))
                assert st == OB_OK
                ref = R.np_keep_rows(seed, ctr + off, rows, T, p).astype(np.uint8).ravel()
                got = out.cpu().numpy()
                bad = int((got != ref).sum())
                assert bad == 0, f"seed {seed} ctr {ctr} off {off} p {p} rows {rows} T {T}: {bad} of {n} keep bits differ"
                if rows == 1:
                    assert np.array_equal(ref, R.np_keep_flat(seed, ctr + off, n, p).astype(np.uint8))


# ---------------------------------------------------------------------------------------
# 3. the d x alignment matrix


@pytest.mark.parametrize("d,off", MATRIX, ids=_IDS)
def test_matrix_fwd(gpu, lib, d, off):
    check_fwd(lib, gpu, ROWS, d, off)


@pytest.mark.parametrize("d,off", MATRIX, ids=_IDS)
def test_matrix_fwd_pair(gpu, lib, d, off):
    check_fwd_pair(lib, gpu, ROWS, d, off)


@pytest.mark.parametrize("d,off", MATRIX, ids=_IDS)
def test_matrix_fwd_amax_i8(gpu, lib, d, off):
    t = inputs(ROWS, d)
    check_amax_i8(lib, gpu, t["x"], t["g"], t["b"], EPS, 1, off, f"rows {ROWS} d {d} off {off} P 1")


@pytest.mark.parametrize("d,off", MATRIX, ids=_IDS)
def test_matrix_bwd(gpu, lib, d, off):
    check_bwd(lib, gpu, ROWS, d, off)


@pytest.mark.parametrize("d,off", MATRIX, ids=_IDS)
def test_matrix_bwd_res_ex(gpu, lib, d, off):
    check_bwd_res_ex(lib, gpu, 39, d, off)  # rows = 3 * T, T = 13, lens = [13, 6, 0]


@pytest.mark.parametrize("d,off", MATRIX, ids=_IDS)
def test_matrix_bwd_pair(gpu, lib, d, off):
    check_bwd_pair(lib, gpu, 39, d, off)


def test_gs_layout_rows_39():
    """the matrix's GradScale case: rows = 3 * T, T = 13, lens = [T, T // 2, 0]"""
    assert gs_layout(39) == (13, [13, 6, 0])


def test_bwd_defer_param_table(gpu, lib):
    """Three LNs of different d write slots 0..2 of one table; one ob_ln_param_table launch
    reduces them: dgamma / dbeta bitwise the immediate (table NULL) result, and within the bar."""
    ds = [4, 143, 512]
    eb = lib.ob_ln_param_entry_bytes()
    table = torch.zeros(3 * eb, dtype=torch.uint8, device=gpu)
    hold, outs = [], []
    for slot, d in enumerate(ds):
        t = inputs(ROWS, d)
        dy, x, g = (f32(t[k], gpu) for k in ("dy", "x", "g"))
        mean, rstd = _stats32(ROWS, d, "std", gpu, 0)
        wsb = lib.ob_layernorm_bwd_workspace(ROWS, d)
        res = {}
        for mode in ("now", "defer"):
            ws = alloc_ws(wsb, gpu)
            dx, dg, db = nans((ROWS, d), gpu), nans(d, gpu), nans(d, gpu)
            st = c_bwd_defer(lib, gpu, dy, x, g, mean, rstd, ROWS, d, None, dx, dg, db, ws, wsb, None,
                             1.0, 0.0, None, 0, None, 0, table if mode == "defer" else None, slot)
            assert st == OB_OK, (d, mode, st)
            res[mode] = (dx, dg, db)
            hold.append((ws, dy, x, g, mean, rstd))
        outs.append(res)
    torch.cuda.synchronize()
    for d, res in zip(ds, outs):  # nothing reduced yet: the deferred dgamma / dbeta are untouched
        assert torch.isnan(res["defer"][1]).all() and torch.isnan(res["defer"][2]).all(), d
    assert lib.ob_ln_param_table(table.data_ptr(), 3, 512, stream(gpu)) == OB_OK
    for d, res in zip(ds, outs):
        w = f"rows {ROWS} d {d}"
        for i, name in enumerate(("dx", "dgamma", "dbeta")):
            bitwise(res["defer"][i], res["now"][i], f"bwd_defer {name} vs immediate {w}")
        dxr, dgr, dbr = ref_bwd(ROWS, d)
        close("bwd_defer", "dx", res["defer"][0], dxr, w)
        rel_l2("bwd_defer", "dgamma", res["defer"][1], dgr, w)
        rel_l2("bwd_defer", "dbeta", res["defer"][2], dbr, w)


# ---------------------------------------------------------------------------------------
# 4. row-count edges

D_EDGE = [8, 68, 143]


@pytest.mark.parametrize("d", D_EDGE)
@pytest.mark.parametrize("rows", [1, 15, 16, 17])
def test_rows_all_kernels(gpu, lib, rows, d):
    check_fwd(lib, gpu, rows, d, 0)
    check_fwd_pair(lib, gpu, rows, d, 0)
    t = inputs(rows, d)
    check_amax_i8(lib, gpu, t["x"], t["g"], t["b"], EPS, 1, 0, f"rows {rows} d {d} P 1")
    check_bwd(lib, gpu, rows, d, 0)
    check_bwd_res_ex(lib, gpu, rows, d, 0)
    check_bwd_pair(lib, gpu, rows, d, 0)


@pytest.mark.parametrize("d", D_EDGE)
def test_rows_8193_backwards(gpu, lib, d):
    """Past the 512-block cap: 32 rows per block, the last block short."""
    rows = 8193
    check_bwd(lib, gpu, rows, d, 0, variants=False)
    check_bwd_res_ex(lib, gpu, rows, d, 0)
    check_bwd_pair(lib, gpu, rows, d, 0)


def test_rows_32785_amax_grid_stride(gpu, lib):
    """2048 * 16 + 17 rows at d = 8: the absmax kernel's 2048 blocks take a second trip for the
    last 17 rows, and the global maximum sits there. LN is scale-invariant per row, so scaling
    a row alone cannot move max|y|; the row is 50 * (+-1) * one-hot at the column c with the
    largest |gamma_c| * sqrt(d - 1) + |beta_c|, signed so that both terms add: that value bounds
    |y| of every row and only a one-hot row reaches it."""
    rows, d = 2048 * 16 + 17, 8
    t = inputs(rows, d)
    x = t["x"].clone()
    g, b = t["g"], t["b"]
    c = int((g.abs() * (d - 1) ** 0.5 + b.abs()).argmax())
    sign = 1.0 if (g[c] * b[c]).item() >= 0 else -1.0
    x[rows - 5] = 0.0
    x[rows - 5, c] = 50.0 * sign
    want = check_amax_i8(lib, gpu, x, g, b, EPS, 1, 0, f"rows {rows} d {d} P 1")
    yr, _, _ = R.ln_fwd(x, g, b, EPS)
    top = int(yr.abs().amax(dim=1).argmax())
    assert top == rows - 5, f"test setup: the maximum is in row {top}, not in the second grid trip"
    assert abs(want.item() - yr.abs().max().item()) <= 1e-5 * yr.abs().max().item() + 1e-6


def test_rows_zero(gpu, lib):
    """rows = 0 on every entry point: status OK, amax written 0, no row output touched (the
    outputs are NaN-filled 16-row buffers). dgamma / dbeta of an immediate reduction are the sum
    over no rows: exactly 0 (onebit_asr/layernorm.py hands them to autograd from torch.empty)."""
    d, cap = 68, 16
    t = inputs(cap, d)
    x, g, b, dy, dres = (f32(t[k], gpu) for k in ("x", "g", "b", "dy", "dres"))
    g2, b2 = f32(t["g2"], gpu), f32(t["b2"], gpu)
    mean, rstd = _stats32(cap, d, "std", gpu, 0)
    rng = rng_tensor(gpu)
    lens = torch.tensor([3], dtype=torch.int32, device=gpu)

    def untouched(*ts):
        for o in ts:
            assert torch.isnan(o).all().item(), "an output was written at rows = 0"

    y, m, r = nans((cap, d), gpu), nans(cap, gpu), nans(cap, gpu)
    assert c_fwd(lib, gpu, x, g, b, 0, d, EPS, y, m, r) == OB_OK
    untouched(y, m, r)
    o = [nans(s, gpu) for s in ((cap, d), cap, cap, (cap, d), cap, cap)]
    assert c_fwd_pair(lib, gpu, x, g, b, g2, b2, 0, d, EPS, EPS2, *o) == OB_OK
    untouched(*o)
    for Pn in (1, 3, 8):
        wsb = lib.ob_layernorm_fwd_amax_workspace(Pn)
        ws = alloc_ws(wsb, gpu)
        amax = nans(8, gpu)
        assert c_fwd_amax(lib, gpu, x, g, b, 0, d, EPS, y, m, r, Pn, amax, ws, wsb) == OB_OK
        untouched(y, m, r, amax[Pn:])
        assert (amax[:Pn].cpu() == 0).all(), f"fwd_amax rows 0 P {Pn}: amax {amax.tolist()}"
        amax, yq = nans(8, gpu), q_out(cap, d, gpu)
        assert c_fwd_i8(lib, gpu, x, g, b, 0, d, EPS, Pn, amax, yq, ws, wsb) == OB_OK
        untouched(amax[Pn:])
        assert (amax[:Pn].cpu() == 0).all() and (yq.cpu() == -128).all()
    wsb = lib.ob_layernorm_bwd_workspace(0, d)
    ws = alloc_ws(wsb, gpu)
    table = torch.full((lib.ob_ln_param_entry_bytes(),), 0xFF, dtype=torch.uint8, device=gpu)

    def params_zero(*ts):
        for o in ts:
            assert (o.cpu() == 0).all(), "dgamma / dbeta over no rows must be exactly 0"

    dx, dg, db, dy2 = nans((cap, d), gpu), nans(d, gpu), nans(d, gpu), nans((cap, d), gpu)
    assert c_bwd(lib, gpu, dy, x, g, mean, rstd, 0, d, dx, dg, db, ws, wsb) == OB_OK
    untouched(dx)
    params_zero(dg, db)
    dg, db = nans(d, gpu), nans(d, gpu)
    assert c_bwd_res(lib, gpu, dy, x, g, mean, rstd, 0, d, dres, dx, dg, db, ws, wsb) == OB_OK
    untouched(dx)
    params_zero(dg, db)
    dg, db = nans(d, gpu), nans(d, gpu)
    assert c_bwd_ex(lib, gpu, dy, x, g, mean, rstd, 0, d, dres, dx, dg, db, ws, wsb, dy2, RSCALE,
                    P_DROP, rng, RNG_OFF, lens, 3) == OB_OK
    untouched(dx, dy2)
    params_zero(dg, db)
    dg, db = nans(d, gpu), nans(d, gpu)
    assert c_bwd_defer(lib, gpu, dy, x, g, mean, rstd, 0, d, dres, dx, dg, db, ws, wsb, dy2, RSCALE,
                       P_DROP, rng, RNG_OFF, lens, 3, table, 0) == OB_OK
    untouched(dx, dy2)
    params_zero(dg, db)  # nothing to defer: reduced at once, the table slot stays as it was
    assert (table.cpu() == 0xFF).all()
    wsb = lib.ob_layernorm_bwd_pair_workspace(0, d)
    ws = alloc_ws(wsb, gpu)
    dg2, db2, dg1, db1 = (nans(d, gpu) for _ in range(4))
    assert c_bwd_pair(lib, gpu, dy, x, g2, mean, rstd, dres, x, g, mean, rstd, 0, d, dx, dg2, db2, dg1,
                      db1, ws, wsb, dy2, RSCALE, P_DROP, rng, RNG_OFF, lens, 3, table, 0, 0) == OB_OK
    untouched(dx, dy2)
    params_zero(dg2, db2, dg1, db1)
    assert (table.cpu() == 0xFF).all()
    # dgamma / dbeta NULL: nothing at all is written
    assert c_bwd(lib, gpu, dy, x, g, mean, rstd, 0, d, dx, None, None, None, 0) == OB_OK
    untouched(dx)
    assert lib.ob_ln_param_table(None, 0, 512, stream(gpu)) == OB_OK
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------
# 5. passes


@pytest.mark.parametrize("d", [144, 63])
@pytest.mark.parametrize("Pn,rpp", [(3, 37), (8, 5), (2, 16)])
def test_passes(gpu, lib, Pn, rpp, d):
    """P > 1: amax[p] == max|y[pass p]| exactly and the int8 image at its own pass's scale.
    Pass k's rows are scaled by 2^k. LN undoes a row's scale unless eps matters, so eps = 1
    with |x| << 1 (y ~ (x - mean) * gamma: the scale shows in y) and beta ~ 0. Each pass's
    last row holds that pass's only maximum M_k and its first row a value F_k with
    M_(k-1) < F_k < M_k: a boundary row credited to the neighbouring pass lowers its own
    pass's maximum or raises the neighbour's."""
    rows = Pn * rpp
    gen = torch.Generator().manual_seed(10 * Pn + d)
    g = torch.randn(d, generator=gen) * 0.5 + 1
    b = torch.randn(d, generator=gen) * 1e-6
    c = int(g.abs().argmax())
    x = torch.randn(rows, d, generator=gen).clamp_(-3.5, 3.5)
    sig = 1e-3 * 2.0 ** torch.arange(Pn, dtype=torch.float32).repeat_interleave(rpp)
    x = x * sig[:, None]
    for k in range(Pn):
        x[k * rpp, c] = 8 * 1e-3 * 2.0 ** k
        x[(k + 1) * rpp - 1, c] = 12 * 1e-3 * 2.0 ** k
    eps = 1.0
    yr, _, _ = R.ln_fwd(x, g, b, eps)
    rowmax = yr.abs().amax(dim=1).view(Pn, rpp)
    assert (rowmax.argmax(dim=1) == rpp - 1).all(), "test setup: a pass's maximum is not in its last row"
    M, F = rowmax[:, -1], rowmax[:, 0]
    assert (F[1:] > M[:-1] * 1.1).all() and (F < M / 1.1).all(), "test setup: M_(k-1) < F_k < M_k"
    assert (rowmax[:, 1:-1].amax(dim=1) < F / 1.1).all(), "test setup: an inner row above the first"
    want = check_amax_i8(lib, gpu, x, g, b, eps, Pn, 0, f"rows {rows} d {d} P {Pn}")
    assert ((want.double() - M).abs() <= 1e-5 * M + 1e-6).all(), (want.tolist(), M.tolist())


# ---------------------------------------------------------------------------------------
# 6. numerics


@pytest.mark.parametrize("d", [63, 144, 512])
def test_zero_rows_among_normal_rows(gpu, lib, d):
    rows, kind = ROWS, "zeros"
    t = inputs(rows, d, kind)
    zr = (t["x"] == 0).all(dim=1)
    assert zr.sum().item() == 5
    x, g, b = (f32(t[k], gpu) for k in ("x", "g", "b"))
    y, mean, rstd = nans((rows, d), gpu), nans(rows, gpu), nans(rows, gpu)
    assert c_fwd(lib, gpu, x, g, b, rows, d, EPS, y, mean, rstd) == OB_OK
    yc, mc, rc = y.cpu(), mean.cpu(), rstd.cpu()
    bitwise(yc[zr], t["b"].expand(5, d), f"y of an all-zero row vs beta, d {d}")
    assert (mc[zr] == 0).all(), mc[zr].tolist()
    want = np.float32(1.0) / np.sqrt(np.float32(EPS), dtype=np.float32)
    ulp = np.spacing(want)
    err = np.abs(rc[zr].numpy().astype(np.float64) - np.float64(want)).max()
    assert err <= ulp, f"rstd of an all-zero row d {d}: |err| {err:.3e} > 1 ulp {ulp:.3e}"
    check_fwd(lib, gpu, rows, d, 0, kind)
    check_bwd(lib, gpu, rows, d, 0, kind, variants=False)


@pytest.mark.parametrize("d", [63, 144, 512])
def test_variance_far_below_eps(gpu, lib, d):
    check_fwd(lib, gpu, ROWS, d, 0, "small")
    check_bwd(lib, gpu, ROWS, d, 0, "small", variants=False)


@pytest.mark.parametrize("d", [63, 144, 512])
def test_offset_mean(gpu, lib, d):
    """x = randn + 30: fp32 itself comes near the bar here, so each bar is max(project bar,
    4 x the error of torch's own fp32 CPU LayerNorm against float64 on the same inputs); the 4
    covers the different summation order (a 16-lane tree here, a vectorised sum there)."""
    rows, kind = ROWS, "off30"
    t = inputs(rows, d, kind)
    x = t["x"].clone().requires_grad_(True)
    w, b = t["g"].clone().requires_grad_(True), t["b"].clone().requires_grad_(True)
    y, mean, rstd = torch.native_layer_norm(x, (d,), w, b, EPS)
    y.backward(t["dy"])
    yr, mr, rr = ref_fwd(rows, d, kind)
    dxr, dgr, dbr = ref_bwd(rows, d, kind)
    e = {"y": (y.detach().double() - yr).abs().max().item(),
         "mean": (mean.detach().double().view(-1) - mr).abs().max().item(),
         "rstd": ((rstd.detach().double().view(-1) - rr).abs() / rr).max().item(),
         "dx": (x.grad.double() - dxr).abs().max().item(),
         "dgamma": ((w.grad.double() - dgr).norm() / dgr.norm()).item(),
         "dbeta": ((b.grad.double() - dbr).norm() / dbr.norm()).item()}
    print(f"\ntorch fp32 CPU LayerNorm vs float64, x = randn + 30, rows {rows} d {d}: "
          + ", ".join(f"{k} {v:.3e}" for k, v in e.items()))
    floors = {k: 4.0 * v for k, v in e.items()}
    check_fwd(lib, gpu, rows, d, 0, kind, floors)
    check_bwd(lib, gpu, rows, d, 0, kind, floors, variants=False)


# ---------------------------------------------------------------------------------------
# 7. argument checks: return codes only, nothing is launched with bad arguments


class _Args:
    """Valid buffers for every entry point at (rows, d); d_buf sizes them for the largest d
    tried, so a call that wrongly went through would still stay inside them."""

    def __init__(self, lib, gpu, rows=6, d=16, d_buf=516):
        self.lib, self.gpu, self.rows, self.d = lib, gpu, rows, d
        z = lambda *s: torch.zeros(*s, device=gpu)  # noqa: E731
        self.x, self.y, self.dy, self.dres, self.dx, self.dy2, self.y2 = (z(rows, d_buf) for _ in range(7))
        self.g, self.b, self.g2, self.b2, self.dg, self.db, self.dg2, self.db2 = (z(d_buf) + 1 for _ in range(8))
        self.mean, self.rstd, self.mean2, self.rstd2 = (z(rows) + 1 for _ in range(4))
        self.amax = z(8)
        self.yq = torch.zeros(rows, d_buf, dtype=torch.int8, device=gpu)
        self.lens = torch.ones(rows, dtype=torch.int32, device=gpu)  # rows ints: lens[row] stays inside
        self.rng = rng_tensor(gpu)
        self.ws = torch.zeros(2 * (2 * 4 * rows * d_buf + 256) + 8 * 2048 * 4, dtype=torch.uint8, device=gpu)
        self.table = torch.zeros(2 * lib.ob_ln_param_entry_bytes(), dtype=torch.uint8, device=gpu)

    def call(self, name, **kw):
        a = dict(x=self.x, y=self.y, dy=self.dy, dres=self.dres, dx=self.dx, dy2=self.dy2, rows=self.rows,
                 d=self.d, P=1, T=2, p=P_DROP, lens=self.lens, wsb=None, g=self.g)
        a.update(kw)
        lib, gpu, rows, d = self.lib, self.gpu, a["rows"], a["d"]
        big = self.ws.numel()
        wsb = a["wsb"]
        gs = (a["dy2"], RSCALE, a["p"], self.rng, RNG_OFF, a["lens"], a["T"])
        if name == "fwd":
            return c_fwd(lib, gpu, a["x"], a["g"], self.b, rows, d, EPS, a["y"], self.mean, self.rstd)
        if name == "fwd_pair":
            return c_fwd_pair(lib, gpu, a["x"], a["g"], self.b, self.g2, self.b2, rows, d, EPS, EPS2,
                              a["y"], self.mean, self.rstd, self.y2, self.mean2, self.rstd2)
        if name == "fwd_amax":
            return c_fwd_amax(lib, gpu, a["x"], a["g"], self.b, rows, d, EPS, a["y"], self.mean, self.rstd,
                              a["P"], self.amax, self.ws, big if wsb is None else wsb)
        if name == "fwd_i8":
            return c_fwd_i8(lib, gpu, a["x"], a["g"], self.b, rows, d, EPS, a["P"], self.amax, self.yq,
                            self.ws, big if wsb is None else wsb)
        head = (a["dy"], a["x"], a["g"], self.mean, self.rstd, rows, d)
        tail = (a["dx"], self.dg, self.db, self.ws, big if wsb is None else wsb)
        if name == "bwd":
            return c_bwd(lib, gpu, *head, *tail)
        if name == "bwd_res":
            return c_bwd_res(lib, gpu, *head, a["dres"], *tail)
        if name == "bwd_ex":
            return c_bwd_ex(lib, gpu, *head, a["dres"], *tail, *gs)
        if name == "bwd_defer":
            return c_bwd_defer(lib, gpu, *head, a["dres"], *tail, *gs, self.table, 0)
        assert name == "bwd_pair"
        return c_bwd_pair(lib, gpu, a["dy"], self.y, self.g2, self.mean2, self.rstd2, a["dres"], a["x"],
                          a["g"], self.mean, self.rstd, rows, d, a["dx"], self.dg2, self.db2, self.dg,
                          self.db, self.ws, big if wsb is None else wsb, *gs, self.table, 0, 1)


_ENTRIES = ["fwd", "fwd_pair", "fwd_amax", "fwd_i8", "bwd", "bwd_res", "bwd_ex", "bwd_defer", "bwd_pair"]


@pytest.fixture(scope="module")
def args(lib, gpu):
    return _Args(lib, gpu)


def test_args_bwd_pair_lens_needs_a_valid_T(args):
    """With dy2 and lens, T < 1 or rows % T != 0 is OB_ERR_SHAPE (as ob_layernorm_bwd_defer):
    the launcher would otherwise index lens[row] past a [B] array. lens here holds rows ints,
    so a call that got through would still read inside the buffer."""
    for T in (0, -1, 4, 7, 2**31):  # rows = 6
        for name in ("bwd_pair", "bwd_defer", "bwd_ex"):
            st = args.call(name, T=T)
            assert st == OB_ERR_SHAPE, f"{name} T {T} rows {args.rows}: status {st}, expected {OB_ERR_SHAPE}"
    lens2 = args.lens.view(torch.uint8)[2:6].data_ptr()
    for name in ("bwd_pair", "bwd_defer", "bwd_ex"):
        assert args.call(name, lens=lens2) == OB_ERR_ALIGN, name
        # lens or dy2 absent: T is not read
        assert args.call(name, lens=None, T=0) == OB_OK, name
        assert args.call(name, dy2=None, T=0) == OB_OK, name
        assert args.call(name, T=3) == OB_OK, name
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", _ENTRIES)
def test_args_d_out_of_range(args, lib, name):
    for d in (0, 513):
        st = args.call(name, d=d)
        assert st == OB_ERR_SHAPE, f"{name} d {d}: status {st}"
    assert args.call(name, rows=-1) == OB_ERR_SHAPE


def test_args_workspace_queries(lib):
    for d in (0, 513):
        assert lib.ob_layernorm_bwd_workspace(6, d) == 0
        assert lib.ob_layernorm_bwd_pair_workspace(6, d) == 0
    assert lib.ob_layernorm_bwd_workspace(-1, 16) == 0
    assert lib.ob_layernorm_bwd_pair_workspace(6, 16) == 2 * lib.ob_layernorm_bwd_workspace(6, 16) > 0
    assert lib.ob_layernorm_fwd_amax_workspace(0) == 0 and lib.ob_layernorm_fwd_amax_workspace(9) == 0
    assert lib.ob_layernorm_fwd_amax_workspace(8) == 8 * lib.ob_layernorm_fwd_amax_workspace(1) > 0
    assert lib.ob_ln_param_table(None, 0, 513, None) == OB_ERR_SHAPE
    assert lib.ob_ln_param_table(None, -1, 512, None) == OB_ERR_SHAPE
    assert lib.ob_ln_param_table(None, 1, 512, None) == OB_ERR_NULL


@pytest.mark.parametrize("name", ["fwd_amax", "fwd_i8"])
def test_args_passes(args, name):
    for Pn in (0, 9, 4, 5):  # rows = 6: 4 and 5 do not divide it
        st = args.call(name, P=Pn)
        assert st == OB_ERR_SHAPE, f"{name} P {Pn} rows {args.rows}: status {st}"
    for Pn in (1, 2, 3, 6):
        assert args.call(name, P=Pn) == OB_OK, (name, Pn)
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", _ENTRIES)
def test_args_pointer_two_bytes_off(args, name):
    fwd = name.startswith("fwd")
    for key in (("x", "y") if fwd else ("dy", "x", "dx")):
        if name == "fwd_i8" and key == "y":
            continue
        st = args.call(name, **{key: getattr(args, key).data_ptr() + 2})
        assert st == OB_ERR_ALIGN, f"{name} {key} + 2 bytes: status {st}"
    if name in ("bwd_res", "bwd_ex", "bwd_defer", "bwd_pair"):
        assert args.call(name, dres=args.dres.data_ptr() + 2) == OB_ERR_ALIGN
    if name in ("bwd_ex", "bwd_defer", "bwd_pair"):
        assert args.call(name, dy2=args.dy2.data_ptr() + 2) == OB_ERR_ALIGN
    if fwd or name == "bwd_pair":
        assert args.call(name, g=args.g.data_ptr() + 2) == OB_ERR_ALIGN


@pytest.mark.parametrize("name", _ENTRIES[2:])
def test_args_workspace_one_short(args, lib, name):
    rows, d = args.rows, args.d
    if name in ("fwd_amax", "fwd_i8"):
        need = lib.ob_layernorm_fwd_amax_workspace(1)
    elif name == "bwd_pair":
        need = lib.ob_layernorm_bwd_pair_workspace(rows, d)
    else:
        need = lib.ob_layernorm_bwd_workspace(rows, d)
    assert need > 0
    st = args.call(name, wsb=need - 1)
    assert st == OB_ERR_WORKSPACE, f"{name} ws_bytes {need - 1} of {need}: status {st}"
    assert args.call(name, wsb=need) == OB_OK, name
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", ["bwd_ex", "bwd_defer", "bwd_pair"])
def test_args_p_drop_one(args, name):
    for p in (1.0, 1.5, -0.1, float("nan")):
        st = args.call(name, p=p)
        assert st == OB_ERR_SHAPE, f"{name} p_drop {p}: status {st}"
