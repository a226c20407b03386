"""The conv module core (csrc/convmod.hip) through its C ABI, at every path of its two
launchers, against float64 (tests/convmod_ref.py: written from the contract in
include/onebit_hip.h, checked on the CPU by tests/test_convmod_ref_cpu.py, which also shows
that float32 alone keeps every case below a quarter of each bar).

Every output and the workspace are NaN-filled before a call; every output carries 64 floats of
a sentinel after its end (the workspace 256 bytes) that must come back unchanged. The
backward's z, g and stats are the device forward's own outputs, as the ABI says.

Bars (the project's: tests/test_layernorm_family_gpu.py, tests/test_convmod_gpu.py):
  v, z, g, du             max|err| <= 1e-5 * max|ref| + 1e-6
  dw_dw, dgamma, dbeta    rel-L2 <= 1e-5
  mean / rstd             against float64 statistics of the device's own z: 1e-6 * max|z| /
                          1e-6 relative (the reduction alone); against the reference:
                          1e-5 * max|z| / 1e-5 relative
  db_dw                   a true zero: max|db_dw| <= 1e-5 * max_c sum_rows |dz_ref|
  dw_dw at K = 1          a true zero (eps = 1e-12 there, convmod_ref.eps_of):
                          max|dw_dw| <= 1e-5 * max_c sum_rows |dz_ref * g_ref|

Matrix (P, B, T, C, K) and how the launchers treat each row. tile_cg: K = 31 and C % 48 / 32 /
16 == 0 -> channel groups of 48 / 32 / 16, used only when pick_tt == 64. pick_tt: the widest
of 64 / 32 / 16 frames whose backward LDS image 4 * (2 * (TT + K - 1) * C + C * K) fits 160 KB.
dw_threads: C * ceil((K + 1) / 8) rounded up to 64, within [256, 1024]. Statistics and the
BatchNorm passes: row-vector kernels when C % 4 == 0 (and C / 4 <= 256), else scalar;
stats_chunks = ceil(rows_pp / 16) capped at 512; rows_chunks = ceil(rows_pp / (8 * row
lanes)), row lanes = 256 / (C / 4), clamped to min(ceil(rows_pp / 16), 512).

  tiles48  (3, 2, 70, 144, 31)   cm_*_tile_kernel<31,48>, three channel groups, two tiles, the
                                 last of 6 frames (weight gradient: remainder loop only), 3 passes
  tiles48  (1, 2, 129, 48, 31)   one group, three tiles, the last of 1 frame
  tiles32  (2, 2, 64, 64, 31)    <31,32>, two groups, T exactly one tile (8 full rounds)
  tiles16  (3, 1, 65, 80, 31)    <31,16> (80 % 48, 80 % 32 != 0), five groups, T = 65
  tiles16  (1, 1, 72, 16, 31)    last tile exactly 8 frames: one full round, no remainder
  tiles48  (1, 64, 1, 48, 31)    T = 1;  (1, 8, 8, 48, 31) T = 8;  (1, 8, 15, 48, 31) T = 15 =
                                 the half-width;  (1, 4, 16, 48, 31) T = 16
  row31    (3, 1, 70, 36, 31)    C % 16 != 0: cm_glu_dw_fwd_kernel<31> / cm_dz / cm_dw_bwd_kernel<31>
                                 / cm_glu_bwd, TT = 64, 256 threads (lower clamp); C % 4 == 0:
                                 row-vector statistics (7 row lanes of 9 groups), 3 passes
  row31    (1, 2, 70, 37, 31)    C % 4 != 0: cm_stats_part / cm_bn_swish_fwd / cm_bn_bwd_part
  row31    (3, 1, 70, 37, 31)    the same with 3 passes (the scalar kernels' pass index)
  row31    (1, 3, 33, 1, 31)     C = 1 (scalar statistics)
  row31    (1, 2, 70, 256, 31)   C % 32 == 0 but LDS at TT = 64 is 224,256 B: TT = 32 (158,720 B),
                                 so no tiles; 1024 threads
  row31    (1, 1, 70, 320, 31)   TT = 16 (157,440 B; 198,400 B at 32); 1280 -> 1024 threads
  generic  (1, 2, 50, 48, 1)     cm_glu_dw_fwd_kernel<0> / cm_dw_bwd_kernel<0>: K = 1 (no halo)
  generic  (1, 2, 70, 48, 3)     K = 3;  (1, 2, 100, 48, 33) K = 33, two tiles
  generic  (1, 1, 200, 16, 127)  K = 127, the widest the ABI takes; four tiles, the last of 8
  generic  (1, 1, 70, 144, 63)   K = 63: TT = 32 (144,576 B; 181,440 B at 64); 1152 -> 1024 threads
  row31    (1, 1, 8200, 5, 31)   scalar statistics, ceil(8200 / 16) = 513 chunks capped at 512
  generic  (1, 1, 130, 1024, 3)  row-vector statistics with one row lane (C / 4 = 256);
                                 rows_chunks 17 clamped to ceil(130 / 16) = 9; TT = 16 with
                                 159,744 B of LDS, 4,096 B below the limit
  tiles48  (3, 1, 1, 48, 31)     one row per pass: launch_convmod_bwd's rows_pp == 1 branch, exact
  row31    (3, 1, 1, 36, 31)     zeros (its own test), with row-vector sums at both widths
Not reached: rows_chunks' 512 cap needs more than 8176 rows per pass at C >= 344 (an input of
5.6 M floats, against the few-second budget of a case here); stats_chunks' cap is reached, and
both caps are the same constant sizing the same workspace. rows_chunks / stats_chunks < 1
cannot happen with rows > 0.
"""
import ctypes

import pytest
import torch

import convmod_ref as R

pytestmark = pytest.mark.gpu

OB_OK, OB_ERR_NULL, OB_ERR_SHAPE, OB_ERR_WORKSPACE, OB_ERR_ALIGN = 0, -1, -2, -4, -5
SENT = -7777.0
N_GUARD = 64

_WORST = {}  # (kernel class, quantity) -> (err / bar, err, bar, where)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if _WORST:
        print("\nconv module core vs float64, worst case per kernel class and quantity "
              "(err, bar, err/bar, where):")
        for (cls, q), (ratio, err, bar, where) in sorted(_WORST.items()):
            print(f"  {cls:12s} {q:9s} {err:.3e}  bar {bar:.3e}  {ratio:.3f}  {where}")


@pytest.fixture(scope="module")
def lib(gpu):
    from onebit_asr import _lib

    return _lib.load()


def _check(cls, q, err, bar, where):
    ratio = err / bar if bar > 0 else (0.0 if err == 0 else float("inf"))
    if (cls, q) not in _WORST or not ratio <= _WORST[(cls, q)][0]:
        _WORST[(cls, q)] = (ratio, err, bar, where)
    assert err <= bar, f"{cls} {q} {where}: err {err:.3e} > bar {bar:.3e}"


def bitwise(a, b, what):
    a, b = a.detach().cpu(), b.detach().cpu()
    same = torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert same, f"{what}: {int((a.view(torch.int32) != b.view(torch.int32)).sum())} of {a.numel()} elements differ"


# ---------------------------------------------------------------------------------------
# device buffers and the raw calls


class Guarded:
    """n floats of NaN followed by 64 sentinel floats."""

    def __init__(self, shape, gpu):
        n = 1
        for s in shape:
            n *= s
        self.buf = torch.full((n + N_GUARD,), float("nan"), device=gpu)
        self.buf[n:] = SENT
        self.t = self.buf[:n].view(*shape)
        self.n = n

    def ptr(self):
        return self.buf.data_ptr()

    def intact(self):
        return bool((self.buf[self.n:] == SENT).all().item())


class Workspace:
    """wsb bytes of 0xFF (NaN as float and as double) and 256 guard bytes of 0xA5."""

    def __init__(self, wsb, gpu):
        self.wsb = int(wsb)
        self.buf = torch.full((self.wsb + 256,), 0xFF, dtype=torch.uint8, device=gpu)
        self.buf[self.wsb:] = 0xA5
        assert self.buf.data_ptr() % 8 == 0

    def ptr(self):
        return self.buf.data_ptr()

    def intact(self):
        return bool((self.buf[self.wsb:] == 0xA5).all().item())


def stream(gpu):
    return torch.cuda.current_stream(gpu).cuda_stream


class Dev:
    """One case's inputs on the device and the three entry points on them."""

    def __init__(self, lib, gpu, t, bias=True):
        self.lib, self.gpu, self.t = lib, gpu, t
        self.P, self.T, self.C, self.K = t["P"], t["T"], t["C"], t["K"]
        self.Bt = t["P"] * t["B"]
        self.rows = self.Bt * self.T
        self.u, self.w, self.gamma, self.beta, self.dv = (t[k].contiguous().to(gpu) for k in
                                                          ("u", "w", "gamma", "beta", "dv"))
        self.b = t["b"].to(gpu) if bias else None
        self.wsb = lib.ob_convmod_workspace(self.P, self.Bt, self.T, self.C, self.K)
        assert self.wsb > 0, "ob_convmod_workspace == 0: the shape is not supported"

    def _dims(self):
        return self.P, self.Bt, self.T, self.C, self.K

    def fwd(self):
        gpu, rows, C = self.gpu, self.rows, self.C
        o = {"z": Guarded((rows, C), gpu), "g": Guarded((rows, C), gpu),
             "stats": Guarded((self.P, C, 2), gpu), "v": Guarded((rows, C), gpu)}
        ws = Workspace(self.wsb, gpu)
        st = self.lib.ob_convmod_fwd(self.u.data_ptr(), self.w.data_ptr(),
                                     self.b.data_ptr() if self.b is not None else None,
                                     self.gamma.data_ptr(), self.beta.data_ptr(), *self._dims(),
                                     self.t["eps"], o["z"].ptr(), o["g"].ptr(), o["stats"].ptr(),
                                     o["v"].ptr(), ws.ptr(), ws.wsb, stream(gpu))
        assert st == OB_OK, f"ob_convmod_fwd status {st}"
        torch.cuda.synchronize()
        for k, x in o.items():
            assert x.intact(), f"forward wrote past the end of {k}"
        assert ws.intact(), "forward wrote past the end of the workspace"
        return o

    def bwd(self, f, table=None, slot=0):
        """ob_convmod_bwd on the forward outputs `f`; with a table, ob_convmod_bwd_defer.
        Returns (outputs, workspace, deferred)."""
        gpu, rows, C, K = self.gpu, self.rows, self.C, self.K
        o = {"du": Guarded((rows, 2 * C), gpu), "dw_dw": Guarded((C, K), gpu),
             "dgamma": Guarded((C,), gpu), "dbeta": Guarded((C,), gpu)}
        if self.b is not None:
            o["db_dw"] = Guarded((C,), gpu)
        ws = Workspace(self.wsb, gpu)
        args = (self.dv.data_ptr(), self.u.data_ptr(), f["z"].ptr(), f["g"].ptr(), f["stats"].ptr(),
                self.w.data_ptr(), self.gamma.data_ptr(), self.beta.data_ptr(), *self._dims(),
                o["du"].ptr(), o["dw_dw"].ptr(), o["db_dw"].ptr() if "db_dw" in o else None,
                o["dgamma"].ptr(), o["dbeta"].ptr(), ws.ptr(), ws.wsb)
        took = ctypes.c_int64(-1)
        if table is None:
            st = self.lib.ob_convmod_bwd(*args, stream(gpu))
        else:
            st = self.lib.ob_convmod_bwd_defer(*args, table.data_ptr(), slot, ctypes.addressof(took),
                                               stream(gpu))
        assert st == OB_OK, f"ob_convmod_bwd status {st}"
        torch.cuda.synchronize()
        for k, x in o.items():
            assert x.intact(), f"backward wrote past the end of {k}"
        assert ws.intact(), "backward wrote past the end of the workspace"
        return o, ws, took.value


def host(f, b):
    """The device outputs as CPU tensors, stats split into mean and rstd [P, C]."""
    out = {k: x.t.cpu() for k, x in list(f.items()) + list(b.items())}
    st = out.pop("stats")
    out["mean"], out["rstd"] = st[..., 0].contiguous(), st[..., 1].contiguous()
    return out


def compare(cls, got, ref, t, where, exact_zero=()):
    """Every quantity of `got` against the float64 run `ref`, and the statistics against the
    float64 statistics of the device's own z."""
    for k, x in got.items():
        assert torch.isfinite(x).all(), f"{cls} {k} {where}: non-finite output"
    for q in exact_zero:
        assert (ref[q] == 0).all(), f"{q} {where}: the reference is not exactly 0"
        assert (got[q] == 0).all(), f"{cls} {q} {where}: expected exact zeros, max {got[q].abs().max().item():.3e}"
    for q, (err, bar) in R.errors(got, ref).items():
        _check(cls, q, err, bar, where)
    P, C = t["P"], t["C"]
    zd = got["z"].double().view(P, -1, C)
    mean = zd.mean(dim=1)
    rstd = 1.0 / torch.sqrt(((zd - mean[:, None]) ** 2).mean(dim=1) + t["eps"])
    _check(cls, "mean/ownz", (got["mean"].double() - mean).abs().max().item(),
           R.STAT_OWN * zd.abs().max().item(), where)
    _check(cls, "rstd/ownz", ((got["rstd"].double() - rstd).abs() / rstd).max().item(), R.STAT_OWN, where)


def run_case(lib, gpu, cls, shape, variant="std", bias=True, exact_zero=()):
    t = R.inputs(*shape, variant)
    ref = R.reference(*shape, variant, bias)
    d = Dev(lib, gpu, t, bias)
    f = d.fwd()
    b, _, _ = d.bwd(f)
    got = host(f, b)
    compare(cls, got, ref, t, f"{shape} {variant}{'' if bias else ' no-bias'}", exact_zero)
    return got, ref, t


# ---------------------------------------------------------------------------------------
# 1. the matrix


@pytest.mark.parametrize("case", R.CASES, ids=R.CASE_IDS)
def test_matrix(gpu, lib, case):
    cls, _, shape = case
    run_case(lib, gpu, cls, shape)


@pytest.mark.parametrize("case", R.ONE_ROW, ids=[c[0] for c in R.ONE_ROW])
def test_one_row_per_pass(gpu, lib, case):
    """P = 3, B = T = 1: every pass normalises a single row. xhat = 0, so du, dw_dw and dgamma
    are exactly 0 and v = swish(beta); rstd = 1/sqrt(eps). (The launcher writes these zeros
    itself: through the dz kernels du was dy's rounding error times rstd, up to 4e-6 here.)
    ob_convmod_bwd_defer has nothing to defer: *deferred == 0, the table slot untouched."""
    cls, _, shape = case
    got, ref, t = run_case(lib, gpu, cls, shape, exact_zero=("du", "dw_dw", "dgamma"))
    d = Dev(lib, gpu, t)
    f = d.fwd()
    table = torch.full((lib.ob_cm_wgrad_entry_bytes(),), 0xFF, dtype=torch.uint8, device=gpu)
    b, _, took = d.bwd(f, table, 0)
    assert took == 0 and (table == 0xFF).all()
    again = host(f, b)
    for k in again:
        bitwise(again[k], got[k], f"{k} bwd_defer vs bwd {shape}")
    bitwise(got["mean"], got["z"].view(3, -1), "mean of a one-row pass vs its z")
    assert (got["v"][0] == got["v"][1]).all() and (got["v"][0] == got["v"][2]).all()


# ---------------------------------------------------------------------------------------
# 2. variants, on the first tiles row and the row-vector whole-row one

_VROWS = R.VARIANT_ROWS
_VIDS = [c[0] for c in _VROWS]


@pytest.mark.parametrize("case", _VROWS, ids=_VIDS)
def test_awkward_gamma_and_constant_channel(gpu, lib, case):
    """gamma 0 in one channel, negative in another; a third channel's depthwise weights are 0:
    its z is the bias in every frame, the variance exactly 0, xhat exactly 0 (mean == bias, v
    one value, dgamma == 0), rstd = 1/sqrt(eps), and its du (exactly 0: dg = sum_j 0 * dz) and
    dw_dw (not 0) still match."""
    cls, _, shape = case
    got, ref, t = run_case(lib, gpu, cls, shape, "awkward")
    C = shape[3]
    c, c0 = t["info"]["const"], t["info"]["gamma0"]
    assert (got["z"][:, c] == t["b"][c]).all() and (ref["z"][:, c] == t["b"][c].double()).all()
    assert (got["mean"][:, c] == t["b"][c]).all() and (ref["mean"][:, c] == t["b"][c].double()).all()
    assert got["dgamma"][c] == 0 and ref["dgamma"][c] == 0  # sum of dy * xhat, xhat == 0
    assert (got["v"][:, c] == got["v"][0, c]).all()
    want = t["eps"] ** -0.5
    err = ((got["rstd"][:, c].double() - want).abs() / want).max().item()
    _check(cls, "rstd/const", err, R.STAT_OWN, f"{shape} awkward")
    for half in (c, C + c):
        assert (got["du"][:, half] == 0).all() and (ref["du"][:, half] == 0).all()
    dw = got["dw_dw"][c].double()
    rel = ((dw - ref["dw_dw"][c]).norm() / ref["dw_dw"][c].norm()).item()
    _check(cls, "dw_dw/const", rel, R.REL_L2, f"{shape} awkward")
    # gamma == 0: dz = gamma * ... is 0, and with it that channel's du and dw_dw
    assert (got["dw_dw"][c0] == 0).all() and (got["du"][:, c0] == 0).all()


@pytest.mark.parametrize("case", _VROWS, ids=_VIDS)
def test_saturated_gates(gpu, lib, case):
    """A tenth of u from {-100, -88.5, -30, 30, 100}: the kernels' sigmoid is 1 / (1 + exp(-x))
    through the hardware exp and reciprocal, and exp(100) overflows float. Everything finite
    (compare asserts it) and within the bars."""
    cls, _, shape = case
    run_case(lib, gpu, cls, shape, "saturated")


@pytest.mark.parametrize("case", _VROWS, ids=_VIDS)
def test_null_bias(gpu, lib, case):
    """b_dw = NULL and db_dw = NULL: the reference run without a bias."""
    cls, _, shape = case
    got, _, _ = run_case(lib, gpu, cls, shape, bias=False)
    assert "db_dw" not in got


# ---------------------------------------------------------------------------------------
# 3. determinism, the deferred finish


@pytest.mark.parametrize("case", [R.CASES[0], R.case("TT16-1024threads")], ids=["tiles48", "row31-TT16"])
def test_run_to_run_bitwise(gpu, lib, case):
    shape = case[2]
    d = Dev(lib, gpu, R.inputs(*shape))
    runs = []
    for _ in range(2):
        f = d.fwd()
        b, _, _ = d.bwd(f)
        runs.append(host(f, b))
    for k in runs[0]:
        bitwise(runs[0][k], runs[1][k], f"{k} run to run {shape}")


def test_deferred_weight_gradient_finish(gpu, lib):
    """ob_convmod_bwd_defer on the CG = 48, 32 and 16 rows writes slots 0..2 of one table and
    leaves dw_dw / db_dw unwritten; one ob_cm_wgrad_table launch finishes all three, bit for
    bit ob_convmod_bwd's result. The C = 36 row runs no tiles: *deferred == 0, finished at once."""
    rows = [R.CASES[0], R.case("2groups-T64"), R.case("5groups-T65")]
    assert [c[0] for c in rows] == ["tiles48", "tiles32", "tiles16"]
    eb = lib.ob_cm_wgrad_entry_bytes()
    assert eb > 0
    table = torch.zeros(3 * eb, dtype=torch.uint8, device=gpu)
    hold, res = [], []
    for slot, (cls, _, shape) in enumerate(rows):
        d = Dev(lib, gpu, R.inputs(*shape))
        f = d.fwd()
        now, _, _ = d.bwd(f)
        later, ws, took = d.bwd(f, table, slot)
        assert took == 1, f"{shape}: *deferred == {took}"
        hold.append((d, f, ws))  # the partials live in ws until the table launch
        res.append((cls, shape, f, now, later))
    for _, shape, _, _, later in res:
        assert torch.isnan(later["dw_dw"].t).all() and torch.isnan(later["db_dw"].t).all(), \
            f"{shape}: dw_dw / db_dw written before the table launch"
    assert lib.ob_cm_wgrad_table(table.data_ptr(), 3, 144 * 32, stream(gpu)) == OB_OK
    torch.cuda.synchronize()
    for cls, shape, f, now, later in res:
        for k in now:
            assert later[k].intact(), f"{shape}: the table launch wrote past the end of {k}"
            bitwise(later[k].t, now[k].t, f"{k} deferred vs immediate {shape}")
        compare(cls + "/defer", host(f, later), R.reference(*shape), R.inputs(*shape), f"{shape} deferred")
    cls, _, shape = R.case("C36-3passes")
    d = Dev(lib, gpu, R.inputs(*shape))
    f = d.fwd()
    now, _, _ = d.bwd(f)
    later, _, took = d.bwd(f, table, 1)
    assert took == 0, f"{shape}: *deferred == {took} on a whole-row shape"
    for k in now:
        bitwise(later[k].t, now[k].t, f"{k} bwd_defer (finished at once) vs bwd {shape}")


# ---------------------------------------------------------------------------------------
# 4. argument checks (nothing is launched), no frames, utterances past the 32-bit offsets


def _raw(lib, gpu, entry, a):
    if entry == "fwd":
        return lib.ob_convmod_fwd(a["u"], a["w"], a["b"], a["gamma"], a["beta"], a["P"], a["Bt"], a["T"],
                                  a["C"], a["K"], 1e-5, a["z"], a["g"], a["stats"], a["v"], a["ws"],
                                  a["wsb"], stream(gpu))
    head = (a["dv"], a["u"], a["z"], a["g"], a["stats"], a["w"], a["gamma"], a["beta"], a["P"], a["Bt"],
            a["T"], a["C"], a["K"], a["du"], a["dw"], a["db"], a["dgamma"], a["dbeta"], a["ws"], a["wsb"])
    if entry == "bwd":
        return lib.ob_convmod_bwd(*head, stream(gpu))
    return lib.ob_convmod_bwd_defer(*head, a["table"], a["slot"], a["took"], stream(gpu))


class _Args:
    """Valid NaN-filled buffers for (P, Bt, T, C, K) = (1, 2, 10, 48, 31), as raw pointers."""

    def __init__(self, lib, gpu, P=1, Bt=2, T=10, C=48, K=31, cap_rows=20):
        rows = cap_rows
        self.out = {"z": Guarded((rows, C), gpu), "g": Guarded((rows, C), gpu),
                    "stats": Guarded((max(P, 1), C, 2), gpu), "v": Guarded((rows, C), gpu),
                    "du": Guarded((rows, 2 * C), gpu), "dw": Guarded((C, K), gpu), "db": Guarded((C,), gpu),
                    "dgamma": Guarded((C,), gpu), "dbeta": Guarded((C,), gpu)}
        self.inp = {"u": torch.randn(rows, 2 * C, device=gpu), "dv": torch.randn(rows, C, device=gpu),
                    "w": torch.randn(C, K, device=gpu), "b": torch.randn(C, device=gpu),
                    "gamma": torch.ones(C, device=gpu), "beta": torch.zeros(C, device=gpu)}
        self.need = lib.ob_convmod_workspace(P, Bt, T, C, K)
        assert self.need > 0
        self.ws = Workspace(self.need + 64, gpu)
        self.table = torch.full((lib.ob_cm_wgrad_entry_bytes(),), 0xFF, dtype=torch.uint8, device=gpu)
        self.took = ctypes.c_int64(7)
        self.a = {k: x.ptr() for k, x in self.out.items()}
        self.a.update({k: x.data_ptr() for k, x in self.inp.items()})
        self.a.update(P=P, Bt=Bt, T=T, C=C, K=K, ws=self.ws.ptr(), wsb=self.need, table=self.table.data_ptr(),
                      slot=0, took=ctypes.addressof(self.took))

    def args(self, **kw):
        return dict(self.a, **kw)

    def untouched(self, but=()):
        torch.cuda.synchronize()
        for k, x in self.out.items():
            assert x.intact(), f"{k}: guard overwritten"
            if k not in but:
                assert torch.isnan(x.t).all(), f"{k} was written"
        assert (self.ws.buf[: self.ws.wsb] == 0xFF).all() and self.ws.intact(), "the workspace was written"
        assert (self.table == 0xFF).all(), "the table was written"


def test_argument_checks_launch_nothing(gpu, lib):
    x = _Args(lib, gpu)
    for entry in ("fwd", "bwd", "defer"):
        assert _raw(lib, gpu, entry, x.args(wsb=x.need - 1)) == OB_ERR_WORKSPACE, entry
        assert _raw(lib, gpu, entry, x.args(ws=x.ws.ptr() + 4)) == OB_ERR_ALIGN, entry
        assert _raw(lib, gpu, entry, x.args(u=None)) == OB_ERR_NULL, entry
        assert _raw(lib, gpu, entry, x.args(K=30)) == OB_ERR_SHAPE, entry
        assert _raw(lib, gpu, entry, x.args(P=2, Bt=3)) == OB_ERR_SHAPE, entry
    assert _raw(lib, gpu, "defer", x.args(slot=-1)) == OB_ERR_SHAPE
    x.untouched()
    assert x.took.value == 7
    assert lib.ob_convmod_workspace(1, 65536, 1, 48, 31) == 0   # Bt > 65535
    assert lib.ob_convmod_workspace(1, 65535, 1, 48, 31) > 0
    assert lib.ob_convmod_workspace(1, 2, 10, 48, 30) == 0      # even K
    assert lib.ob_convmod_workspace(1, 2, 10, 48, 129) == 0     # K > 127
    assert lib.ob_convmod_workspace(2, 3, 10, 48, 31) == 0      # Bt % P != 0
    assert lib.ob_convmod_workspace(1, 2, 10, 384, 31) == 0     # no tile fits: 188,928 B at TT = 16
    assert lib.ob_convmod_workspace(1, 2, 10, 320, 31) > 0


@pytest.mark.parametrize("C", [48, 36], ids=["tiles", "whole-row"])
@pytest.mark.parametrize("P,Bt,T", [(1, 0, 10), (3, 0, 10), (1, 2, 0)], ids=["Bt0", "Bt0-P3", "T0"])
def test_backward_without_frames(gpu, lib, P, Bt, T, C):
    """Bt * T == 0: OB_OK; dw_dw, db_dw, dgamma, dbeta are sums over nothing, exactly 0;
    *deferred = 0; du, the workspace and the table are not touched. (The forward returns
    OB_OK and writes nothing.)"""
    x = _Args(lib, gpu, P=P, Bt=Bt, T=T, C=C)
    assert _raw(lib, gpu, "fwd", x.args()) == OB_OK
    x.untouched()
    params = ("dw", "db", "dgamma", "dbeta")
    for entry in ("bwd", "defer"):
        for k in params:
            x.out[k].t.fill_(float("nan"))
        assert _raw(lib, gpu, entry, x.args()) == OB_OK, entry
        x.untouched(but=params)
        for k in params:
            assert (x.out[k].t == 0).all(), f"{entry} {k}: not exactly 0"
        if entry == "defer":
            assert x.took.value == 0
    # db_dw NULL: the other three still zeroed
    for k in params:
        x.out[k].t.fill_(float("nan"))
    assert _raw(lib, gpu, "bwd", x.args(db=None)) == OB_OK
    x.untouched(but=params)
    assert torch.isnan(x.out["db"].t).all()
    for k in ("dw", "dgamma", "dbeta"):
        assert (x.out[k].t == 0).all(), k


def test_utterance_past_32bit_offsets_is_refused(gpu, lib):
    """The channel-split tiles address one utterance through 32-bit byte offsets; the largest
    they form is below 8 * C * (T + 7) (the backward's gate access of a register window that
    runs up to 7 frames past T). A shape where that passes 2^31 is OB_ERR_SHAPE before any
    pointer is read: nothing is allocated or launched here. The whole-row kernels index in 64
    bits and keep taking such a T."""
    C = 48
    t_max = 2**31 // (8 * C) - 7
    assert 8 * C * (t_max + 7) <= 2**31 < 8 * C * (t_max + 8)
    assert lib.ob_convmod_workspace(1, 1, t_max, C, 31) > 0
    assert lib.ob_convmod_workspace(1, 1, t_max + 1, C, 31) == 0
    assert lib.ob_convmod_workspace(3, 6, t_max + 1, C, 31) == 0
    assert lib.ob_convmod_workspace(1, 1, t_max + 1, 36, 31) > 0   # whole-row kernels
    assert lib.ob_convmod_workspace(1, 1, t_max + 1, C, 33) > 0    # generic width: whole-row
    assert lib.ob_convmod_workspace(1, 1, 2**31 // (8 * 144) - 6, 144, 31) == 0
    null = dict.fromkeys(("u", "w", "b", "gamma", "beta", "z", "g", "stats", "v", "dv", "du", "dw", "db",
                          "dgamma", "dbeta", "ws", "table", "took"))
    null.update(P=1, Bt=1, T=t_max + 1, C=C, K=31, wsb=0, slot=0)
    for entry in ("fwd", "bwd", "defer"):
        assert _raw(lib, gpu, entry, null) == OB_ERR_SHAPE, entry
