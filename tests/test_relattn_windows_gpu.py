"""The prefetch-window specialisations of the attention forward and query-side backward
(relattn_fwd_kernel / relattn_bwd_kernel with WIN, the default where every key tile of the
kernel's tile count is live) against the general kernels they stand in for, reached through
the process-wide switch ``ob_relattn_set_windows`` (bit 0 the backward, bit 1 the forward) --
the yardstick is the unchanged kernel, not the code under test.

Forward: ob_relattn_fwd three times from the same inputs through the C ABI in this process,
mask 0, 3, 3. Before every call ctx and the whole saved state are NaN; 64 sentinel floats
follow both and must come back unchanged. ctx and the saved probability tiles of 0 / 3 and of
3 / 3 must be equal bit for bit (torch.equal, so none is NaN, and once more as int32: a zero's
sign counts); the rest of the saved state is compared as int32 (the probability path leaves
it as it was).

Backward: ob_relattn_bwd three times from one saved forward state, mask 0, 3, 3. Before every
call the six outputs and the workspace are NaN; sentinels follow every output (256 guard bytes
the workspace). dq, dk, dv, dpos, du and dvb must be equal bit for bit, as above.

Shapes: the smallest at which each path can go wrong. A key tile is 16 keys, a query tile 64
queries of four waves; the kernels are built for NTT = 16 tiles (T <= 256) and 32 (above), and
the specialisations run where ceil(T / 16) == NTT:
  T = 1, 15, 16, 17        dead tiles, a partial tile, an exact one          (general kernels)
  T = 63, 64, 65           the query-tile edge; a second query tile of one row (general)
  T = 129, 240             dead waves in the last query tile; nt = 15          (general)
  T = 241, 249, 255, 256   nt == NTT = 16: one key / 9 / 15 / 16 in the last tile, the last
                           query tile with rows past T                  (the specialisations)
  T = 257, 272             NTT = 32 with dead tiles                            (general)
  T = 511, 512             nt == NTT = 32                               (the specialisations)
crossed with (Bt, P) = (1, 1), (3, 3), H = 1 and 4, dropout 0 and 0.1, full and ragged lengths
(with a length 0 row and a length 1 row) at d = 36, and three of those combinations at each
other head width the dispatch instantiates (16, 32, 64).

Float64: one case per T class, mask 3, against the float64 restatement of the reference ops
(relattn_ref.py), at the bars of test_relattn_gpu.py: d = 36, three passes, ragged lengths,
dropout 0.1 -- except T = 1, which is that file's own T = 1 case (Bt 2, P 1, H 4, d 16, lengths
1 and 0). With one key the softmax is 1 and the true dq is exactly 0, so its bound is the bars'
absolute floor of 1e-6 alone, while the kernels form dS' from the difference of two fp32
evaluations of dO . v (dP * keep / (1 - p) and delta = dO . ctx) that agree only to a few ulp
of |dO . v|: at d = 36 that product reaches ~15 over the case's rows and heads, and a few
6e-8 * 15 / sqrt(36) times |k| up to ~3 is about the floor itself (the general kernel, which
T = 1 runs under either mask, gave 1.03e-6 at d = 36, Bt 3); at d = 16 it stays well inside.
"""
import pytest
import torch

import relattn_ref as R

pytestmark = pytest.mark.gpu

SENT = -7777.0
N_GUARD = 64
T_ALL = [1, 15, 16, 17, 63, 64, 65, 129, 240, 241, 249, 255, 256, 257, 272, 511, 512]
T_F64 = [1, 17, 64, 249, 257]
HEAD_WIDTHS = [36, 16, 32, 64]  # OB_RA_DISPATCH: d = 16, 32, 36, else (64)
OUTS = ("dq", "dk", "dv", "dpos", "du", "dvb")


def _combos(d):
    """(Bt, P, H, p, ragged)"""
    if d == 36:
        return [(bt, P, H, p, rg) for bt, P in ((1, 1), (3, 3)) for H in (1, 4)
                for p in (0.0, 0.1) for rg in (False, True)]
    return [(1, 1, 1, 0.0, False), (3, 3, 4, 0.1, False), (3, 3, 4, 0.1, True)]


class Guarded:
    """n floats followed by 64 sentinel floats."""

    def __init__(self, n, gpu):
        self.buf = torch.empty(n + N_GUARD, device=gpu)
        self.buf[n:] = SENT
        self.t = self.buf[:n]
        self.n = n

    def nan(self):
        self.t.fill_(float("nan"))

    def intact(self):
        return bool((self.buf[self.n:] == SENT).all().item())


@pytest.fixture(scope="module")
def lib(gpu):
    from onebit_asr import _lib

    lib = _lib.load()
    prev_mode = lib.ob_relattn_set_bwd_mode(0)  # the probability path holds both kernels
    prev_win = lib.ob_relattn_set_windows(-1)
    yield lib
    lib.ob_relattn_set_bwd_mode(prev_mode)
    lib.ob_relattn_set_windows(prev_win)


def _lens(bt, t, H, ragged):
    if not ragged:
        return [t] * bt
    if bt == 1:
        return [(t + 1) // 2]
    return [0, t, 1] if H == 1 else [1, (t + 1) // 2, 0]


def _same(a, b, what):
    assert torch.equal(a, b), f"{what}: {int((a != b).sum())} of {a.numel()} elements differ"
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{what}: differ in a zero's sign"


def _run(lib, gpu, bt, P, t, H, d, p, ragged):
    """fwd with mask 0, 3, 3 from the same inputs, then bwd with mask 0, 3, 3 from the first
    forward's saved state; asserts the parity of both."""
    from onebit_asr import _lib

    c = H * d
    g = torch.Generator(device=gpu).manual_seed(1000 * t + 10 * d + bt)
    mk = lambda *s: torch.randn(*s, device=gpu, generator=g)  # noqa: E731
    q, k, v, do = mk(bt, t, c), mk(bt, t, c), mk(bt, t, c), mk(bt, t, c)
    pos, u, vb = mk(P, t, c), mk(H, d) * 0.1, mk(H, d) * 0.1
    lens = torch.tensor(_lens(bt, t, H, ragged), dtype=torch.int32, device=gpu)
    rng = torch.tensor([1234, 1], dtype=torch.int64, device=gpu)
    n_saved = lib.ob_relattn_saved_elems(bt, t, H, d)
    tail = n_saved - lib.ob_relattn_probs_elems(bt, t, H)  # the probability tiles end the state
    saved, ctx = Guarded(n_saved, gpu), Guarded(bt * t * c, gpu)
    s = _lib.stream_of(q)
    where = f"Bt {bt} P {P} T {t} H {H} d {d} p {p} lens {lens.tolist()}"

    fw = []
    for mask in (0, 3, 3):
        saved.nan()
        ctx.nan()
        lib.ob_relattn_set_windows(mask)
        _lib.check(lib.ob_relattn_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), pos.data_ptr(),
                                      u.data_ptr(), vb.data_ptr(), lens.data_ptr(), bt, P, t, H, d, p,
                                      rng.data_ptr(), 0, saved.buf.data_ptr(), None,
                                      ctx.buf.data_ptr(), s), "ob_relattn_fwd")
        assert ctx.intact(), f"{where}: mask {mask}: the sentinel after ctx was overwritten"
        assert saved.intact(), f"{where}: mask {mask}: the sentinel after the saved state was overwritten"
        fw.append((ctx.t.clone(), saved.t.clone()))
    for (c0, s0), (c1, s1), tag in ((fw[0], fw[1], "mask 0 vs 3"), (fw[1], fw[2], "two mask 3 runs")):
        _same(c0, c1, f"{where}: ctx {tag}")
        _same(s0[tail:], s1[tail:], f"{where}: probability tiles {tag}")
        assert torch.equal(s0[:tail].view(torch.int32), s1[:tail].view(torch.int32)), \
            f"{where}: the saved state in front of the tiles, {tag}"

    ctx0, saved0 = fw[0]
    wsb = lib.ob_relattn_bwd_workspace(bt, t, H, d)
    ws = torch.empty(wsb + 256, dtype=torch.uint8, device=gpu)
    outs = {n: Guarded(sz, gpu) for n, sz in (("dq", bt * t * c), ("dk", bt * t * c),
                                              ("dv", bt * t * c), ("dpos", P * t * c),
                                              ("du", H * d), ("dvb", H * d))}
    bw = []
    for mask in (0, 3, 3):
        for o in outs.values():
            o.nan()
        ws[:wsb] = 0xFF  # NaN as float
        ws[wsb:] = 0xA5
        lib.ob_relattn_set_windows(mask)
        _lib.check(lib.ob_relattn_bwd(do.data_ptr(), ctx0.data_ptr(), q.data_ptr(), k.data_ptr(),
                                      v.data_ptr(), pos.data_ptr(), u.data_ptr(), vb.data_ptr(),
                                      lens.data_ptr(), bt, P, t, H, d, p, rng.data_ptr(), 0,
                                      saved0.data_ptr(), n_saved,
                                      *(outs[n].buf.data_ptr() for n in OUTS),
                                      ws.data_ptr(), wsb, s), "ob_relattn_bwd")
        for n, o in outs.items():
            assert o.intact(), f"{where}: mask {mask}: the sentinel after {n} was overwritten"
        assert bool((ws[wsb:] == 0xA5).all().item()), f"{where}: mask {mask}: workspace guard"
        bw.append({n: o.t.clone() for n, o in outs.items()})
    for n in OUTS:
        _same(bw[0][n], bw[1][n], f"{where}: {n} mask 0 vs 3")
        _same(bw[1][n], bw[2][n], f"{where}: {n} two mask 3 runs")


@pytest.mark.parametrize("d", HEAD_WIDTHS)
@pytest.mark.parametrize("t", T_ALL)
def test_windows_same_bits_as_the_general_kernels(lib, gpu, t, d):
    for bt, P, H, p, ragged in _combos(d):
        _run(lib, gpu, bt, P, t, H, d, p, ragged)


@pytest.mark.parametrize("t", T_F64)
def test_windows_match_float64(lib, gpu, t):
    """One case per T class, dropout 0.1, ragged lengths, mask 3 (T = 1: see the module's text)."""
    from onebit_asr import attention as at

    bt, P, H, d, p = (2, 1, 4, 16, 0.1) if t == 1 else (3, 3, 4, 36, 0.1)
    lib.ob_relattn_set_windows(3)
    assert lib.ob_relattn_set_windows(-1) == 3
    q, k, v, pos, u, vb = R.inputs(bt, P, t, H, d, seed=bt * 1000 + t)
    lens_t = torch.tensor([1, 0] if t == 1 else [1, t, (t + 1) // 2])
    dev = [x.to(gpu).requires_grad_() for x in (q, k, v, pos, u, vb)]
    ctx = at.rel_pos_attention(*dev, lens_t.to(gpu), H, dropout_p=p)
    rng, off = at.LAST_RNG[torch.device(gpu)]  # the state + offset this call used
    keep = at.dropout_mask((bt, H, t, t), p, rng, off).cpu()
    gout = torch.randn(bt, t, H * d, generator=torch.Generator().manual_seed(7))
    ctx.backward(gout.to(gpu))

    ref_in = [x.double().requires_grad_() for x in (q, k, v, pos, u, vb)]
    rctx, _ = R.ref(*ref_in, lens_t, H, keep=keep, p=p)
    rctx.backward(gout.double())
    R.close(ctx.detach(), rctx.detach(), R.CTX_BAR, "ctx")
    for name, a, b in zip(OUTS, dev, ref_in):
        R.close(a.grad, b.grad, R.GRAD_BAR, f"T {t} {name}")


def test_windows_switch(lib):
    """Returns the previous mask; 0 .. 3 set it, anything else only queries (the module fixture
    restores what it found)."""
    start = lib.ob_relattn_set_windows(-1)
    assert 0 <= start <= 3
    try:
        assert lib.ob_relattn_set_windows(0) == start
        assert lib.ob_relattn_set_windows(4) == 0 and lib.ob_relattn_set_windows(-1) == 0
        assert lib.ob_relattn_set_windows(2) == 0 and lib.ob_relattn_set_windows(7) == 2
        assert lib.ob_relattn_set_windows(1) == 2 and lib.ob_relattn_set_windows(-5) == 1
        assert lib.ob_relattn_set_windows(3) == 1 and lib.ob_relattn_set_windows(-1) == 3
    finally:
        lib.ob_relattn_set_windows(start)
    assert lib.ob_relattn_set_windows(-1) == start
