"""Conv2dSubsampling's convolutions (csrc/subsample.hip) through the C ABI (ob_subsample_pack,
ob_subsample_fwd, ob_subsample_bwd_workspace, ob_subsample_bwd), at every launch path, against
float64 (tests/subsample_ref.py: written from the contract in include/onebit_hip.h, checked on
the CPU by tests/test_subsample_ref_cpu.py, which also shows that float32 alone, masks pinned,
stays below 0.08 of each bar at every row here).

Y1, Y2, the four gradients, the weight image and the workspace are NaN-filled (0xFF bytes)
before a call; every output carries 64 sentinel floats after its end (the image and the
workspace 256 bytes) that must come back unchanged; every output must be finite. The backward
receives the device forward's own Y1 and Y2, as in production.

Masks. A ReLU tie that the device and float64 decide differently moves a gradient by one whole
term (tests/test_subsample_ref_cpu.py flips one and sees db0 move by over ten times its bar),
which is no arithmetic error of either. So the reference's gradients use m1 = Y1_dev > 0 and
m2 = Y2_dev > 0, after the test has asserted that these equal the float64 masks wherever
|pre_ref| exceeds the forward bar of that tensor. The report says how many elements lie inside that band and how many differ
there. The dgrad epilogue does not read Y1: it recomputes relu'(Y1) from X, W0 and b0; where
that disagrees with Y1 > 0 in one element, dW0 / db0 miss their bars by about two decades.

Bars (the project's; the gradients now per element as well):
  Y1, Y2                 max|err| <= 1e-5 * max|ref| + 1e-6
  dW0, db0, dW2, db2     rel-L2 <= 1e-5 and max|err| <= 1e-5 * max|ref|

Matrix (B, T, F, C); M = B T2 F2 forward rows. subsample_ref.plan restates the launch
arithmetic and subsample_ref.check_plan asserts each row's property, so a changed cap or tile
size reports that the coverage moved.
  small   (3, 39, 83, C), C in {48, 64, 96, 144}: launch_gemm6<3 / 4 / 6 / 9> and ss_wgrad<3,1,1> /
          <2,2,2> / <3,2,2> / <3,3,3>; T1 = 19 and F1 = 41 odd, so the four dgrad classes have four
          sizes; M = 540, last tile of 28 rows
  small   T in {7..10} x F in {7..10} at (2, ., ., 48), M = 2: all 16 combinations of a last row /
          column of X and of Y1 that no window reads (dgrad's t2 < T2, f2 < F2 guards), F2 = 1;
          T in {35..38} x F = 80 at C = 144
  rows    (1, 7, 7, C): M = 1; dgrad classes of 4 / 2 / 2 / 1 rows, all but 4 of the dgrad blocks
          have no tile and must write zero partials for ss_w0_finish_kernel
          (2, 35, 35, 64): M = 128 = one full tile;  (3, 175, 7, 96): M = 129, last tile of one row;
          (4, 23, 31, 144): M = 140, last tile of 12 rows (within one 16-row wave fragment)
  wgrad   rows_per_chunk = 32 ceil(M / 896):  (1, 11, 47, 48) M = 22, one chunk of one partial step;
          (4, 59, 67, 64) M = 896, 28 one-step chunks;  (3, 55, 95, 48 and 144) M = 897, 15 chunks,
          the last of one row;  (4, 67, 67, 64) M = 1024, 16 chunks;  (3, 59, 103, 48) M = 1050, 17
          chunks (the finish kernel keeps 16 loads in flight);  (5, 83, 83, 64) 3 steps a chunk,
          (6, 83, 103, 48) 4, (4, 167, 103, 64 and 144) 5: the ra / rb rotation at s + 3, s + 4
  shipped (16, 1000, 80, C) for the four C: 592 forward tiles on 512 blocks (blocks of one and of
          two tiles: the tile loop, the tiles * L / nblk split), every dgrad class 3 to 7 tiles
          per block (the barrier between a tile's epilogue and the next tile's B store, the w0acc
          running sums), conv0 2 to 6 grid-stride passes, wgrad 85 steps a chunk
  int     X, b0, dY2 in {-2..2}, W0, W2 in {-1, 0, 1} (a tenth of W2 non-zero), b2 in {-3..3} at
          (3, 23, 31, 48) and (2, 25, 33, 144): every sum an integer below 2^24, so all six
          outputs equal float64 bit for bit, no mask pinning; 10 % of pre1 and 1 to 3 % of pre2
          are exact ties (pre == 0): `>` against `>=` in conv0, in the output mask and in the
          dgrad recompute
Not reachable: ss_pack_kernel's 4096-block cap (C = 144 packs 11,808 slots * 16 units = 738
blocks of 256), and a dgrad class without rows (T, F >= 7 give T1, F1 >= 3).
"""
import time

import pytest
import torch

import subsample_ref as R

pytestmark = pytest.mark.gpu

OB_OK = 0
SENT = -7777.0
N_GUARD = 64

_WORST = {}  # (class, quantity) -> (err / bar, err, bar, where)
_BAND = {}   # (class, tensor) -> [elements, in the band, differing in the band]
_WALL = {}   # shape -> (device calls s, whole case s)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if _WORST:
        print("\nsubsampling convolutions vs float64, worst case per class and quantity "
              "(err, bar, err/bar, where):")
        for (cls, q), (ratio, err, bar, where) in sorted(_WORST.items()):
            print(f"  {cls:8s} {q:8s} {err:.3e}  bar {bar:.3e}  {ratio:.3f}  {where}")
    if _BAND:
        print("ReLU tie bands (|pre_ref| <= the forward bar): elements, inside, differing inside")
        for (cls, q), (n, inside, differ) in sorted(_BAND.items()):
            print(f"  {cls:8s} {q:4s} {n:12d} {inside:8d} {differ:6d}")
    for shape, (dev, whole) in _WALL.items():
        print(f"  wall {shape}: device calls {dev:.2f} s, whole case {whole:.2f} s")


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
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
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


class Bytes:
    """n bytes of 0xFF (NaN as float) and 256 guard bytes of 0xA5."""

    def __init__(self, n, gpu):
        self.n = int(n)
        self.buf = torch.full((self.n + 256,), 0xFF, dtype=torch.uint8, device=gpu)
        self.buf[self.n:] = 0xA5
        assert self.buf.data_ptr() % 16 == 0

    def ptr(self):
        return self.buf.data_ptr()

    def intact(self):
        return bool((self.buf[self.n:] == 0xA5).all().item())


def stream(gpu):
    return torch.cuda.current_stream(gpu).cuda_stream


class Dev:
    """One case's inputs on the device and the entry points on them."""

    def __init__(self, lib, gpu, t, shape):
        self.lib, self.gpu = lib, gpu
        self.B, self.T, self.F, self.C = shape
        self.T1, self.F1, self.T2, self.F2 = R.dims(self.T, self.F)
        self.x, self.w0, self.b0, self.w2, self.b2, self.dy2 = (
            t[k].contiguous().to(gpu) for k in ("x", "w0", "b0", "w2", "b2", "dy2"))
        self.wsb = lib.ob_subsample_bwd_workspace(*shape)
        assert self.wsb > 0, "ob_subsample_bwd_workspace == 0: the shape is not supported"
        self.img = Bytes(lib.ob_subsample_image_bytes(self.C), gpu)
        st = lib.ob_subsample_pack(self.w2.data_ptr(), self.C, self.img.ptr(), stream(gpu))
        assert st == OB_OK, f"ob_subsample_pack status {st}"
        torch.cuda.synchronize()
        assert self.img.intact(), "the packer wrote past the end of the image"

    def _dims(self):
        return self.B, self.T, self.F, self.C

    def fwd(self):
        gpu, B, C = self.gpu, self.B, self.C
        o = {"Y1": Guarded((B, self.T1, self.F1, C), gpu), "Y2": Guarded((B, self.T2, self.F2, C), gpu)}
        st = self.lib.ob_subsample_fwd(self.x.data_ptr(), *self._dims(), self.w0.data_ptr(),
                                       self.b0.data_ptr(), self.img.ptr(), self.b2.data_ptr(),
                                       o["Y1"].ptr(), o["Y2"].ptr(), stream(gpu))
        assert st == OB_OK, f"ob_subsample_fwd status {st}"
        torch.cuda.synchronize()
        for k, x in o.items():
            assert x.intact(), f"forward wrote past the end of {k}"
        assert self.img.intact(), "forward wrote past the end of the image"
        return o

    def bwd(self, f):
        gpu, C = self.gpu, self.C
        o = {"dW0": Guarded((C, 1, 3, 3), gpu), "db0": Guarded((C,), gpu),
             "dW2": Guarded((C, C, 3, 3), gpu), "db2": Guarded((C,), gpu)}
        ws = Bytes(self.wsb, gpu)
        st = self.lib.ob_subsample_bwd(self.x.data_ptr(), self.w0.data_ptr(), self.b0.data_ptr(),
                                       f["Y1"].ptr(), f["Y2"].ptr(), self.dy2.data_ptr(), *self._dims(),
                                       self.img.ptr(), o["dW0"].ptr(), o["db0"].ptr(), o["dW2"].ptr(),
                                       o["db2"].ptr(), ws.ptr(), ws.n, stream(gpu))
        assert st == OB_OK, f"ob_subsample_bwd status {st}"
        torch.cuda.synchronize()
        for k, x in list(o.items()) + list(f.items()):
            assert x.intact(), f"backward wrote past the end of {k}"
        assert ws.intact(), "backward wrote past the end of the workspace"
        return o

    def run(self):
        """Forward and backward; the outputs as CPU tensors."""
        f = self.fwd()
        b = self.bwd(f)
        return {k: x.t.cpu() for k, x in list(f.items()) + list(b.items())}


def pinned_masks(cls, got, f, where):
    """m1 = Y1_dev > 0, m2 = Y2_dev > 0, after asserting that they are the float64 masks wherever
    |pre_ref| exceeds the forward bar of that tensor."""
    masks = []
    for y, pre, m in (("Y1", "pre1", "m1"), ("Y2", "pre2", "m2")):
        dev = got[y] > 0
        band = f[pre].abs() <= R.fwd_bar(f[y])
        differ = dev != f[m]
        outside = int((differ & ~band).sum())
        row = _BAND.setdefault((cls, y), [0, 0, 0])
        row[0] += dev.numel()
        row[1] += int(band.sum())
        row[2] += int((differ & band).sum())
        assert outside == 0, f"{cls} {y} {where}: {outside} mask elements differ outside the tie band"
        masks.append(dev)
    return masks


def run_case(lib, gpu, cls, shape):
    t = R.inputs(*shape)
    where = str(shape)
    t0 = time.perf_counter()
    got = Dev(lib, gpu, t, shape).run()
    t1 = time.perf_counter()
    for k, x in got.items():
        assert torch.isfinite(x).all(), f"{cls} {k} {where}: non-finite output"
    f = R.forward(t)
    for q, (err, bar) in R.errors(got, f, R.FWD).items():
        _check(cls, q, err, bar, where)
    m1, m2 = pinned_masks(cls, got, f, where)
    ref = R.backward(t, f, m1, m2)
    for k in R.GRADS:
        assert got[k].shape == ref[k].shape
        if ref[k].norm().item() == 0.0:
            assert (got[k] == 0).all(), f"{cls} {k} {where}: expected exact zeros"
    for q, (err, bar) in R.errors(got, ref, R.GRADS).items():
        _check(cls, q, err, bar, where)
    return t1 - t0, time.perf_counter() - t0


# ---------------------------------------------------------------------------------------
# 1. the matrix


@pytest.mark.parametrize("case", R.CASES, ids=R.CASE_IDS)
def test_matrix(gpu, lib, case):
    cls, name, shape = case
    R.check_plan(cls, name, shape)
    wall = run_case(lib, gpu, cls, shape)
    if cls == "shipped":
        _WALL[shape] = wall


# ---------------------------------------------------------------------------------------
# 2. exact integers


@pytest.mark.parametrize("shape", R.INT_CASES, ids=str)
def test_integer_inputs_bit_for_bit(gpu, lib, shape):
    """Every product and sum is an integer below 2^24 (asserted on the reference), the bf16 hi
    plane holds every GEMM operand and the mid and lo planes are zero: all six outputs equal
    float64 exactly, ties at pre == 0 included, with the reference's own masks."""
    t = R.inputs(*shape, "int")
    ref = R.run(t, abs_sums=True)
    assert max(ref["abs"].values()) < 2 ** 24
    assert (ref["pre1"] == 0).any() and (ref["pre2"] == 0).any()
    got = Dev(lib, gpu, t, shape).run()
    for k in R.FWD + R.GRADS:
        diff = got[k].double() != ref[k]
        assert not diff.any(), (f"int {k} {shape}: {int(diff.sum())} of {diff.numel()} elements differ, "
                                f"max |err| {(got[k].double() - ref[k]).abs().max().item():.0f}")
        _check("int", k, 0.0, 0.0, str(shape))


# ---------------------------------------------------------------------------------------
# 3. determinism


@pytest.mark.parametrize("name", ["C144", "M897-15chunks-last1"])
def test_run_to_run_bitwise(gpu, lib, name):
    _, _, shape = R.case(name)
    t = R.inputs(*shape)
    runs = [Dev(lib, gpu, t, shape).run() for _ in range(2)]
    for k in runs[0]:
        bitwise(runs[0][k], runs[1][k], f"{k} run to run {shape}")
