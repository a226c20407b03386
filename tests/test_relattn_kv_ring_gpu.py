"""The key-side attention backward as a two-stage LDS ring (relattn_bwd_kv_ring_kernel, the
default) against the kernel it replaces (relattn_bwd_kv_kernel), reached through the
process-wide switch ``ob_relattn_set_kv_ring`` -- the yardstick is the unchanged kernel, not
the code under test.

Each case runs ob_relattn_fwd once and then ob_relattn_bwd three times from the same saved
state, all through the C ABI in this process: switch off, on, on. Before every backward the
six outputs and the workspace are NaN; 64 sentinel floats follow every output (256 guard
bytes the workspace) and must come back unchanged. dk, dv, dpos, dq, du and dvb of off / on
and of on / on must be equal bit for bit (torch.equal, so none is NaN either).

Shapes: the smallest at which the ring can go wrong. A stage is 16 queries, the stages go in
pairs (the replaced kernel's 32-query chunks), a key tile is 64 keys:
  T = 1, 5, 15, 16, 17     one stage, a partial one, an exact one
  T = 31, 32, 33           the pair edge
  T = 47, 48, 49           three stages: the ring wraps
  T = 63, 64, 65           the key-tile edge; a second key tile of one key
  T = 129, 249             odd T: partial key quads and the row-0 gather on a long run
crossed with (Bt, P) = (1, 1), (3, 3), (6, 3), H = 1 and 4, every head width the dispatch
instantiates (36 first, 16, 32, 64), dropout 0 and 0.1, full and ragged (down to 1) lengths.

Float64: one case per T class, switch on, against the float64 restatement of the reference
ops (relattn_ref.py), at the bars of test_relattn_gpu.py.
"""
import pytest
import torch

import relattn_ref as R

pytestmark = pytest.mark.gpu

SENT = -7777.0
N_GUARD = 64
T_CLASSES = [(1, 5, 15, 16, 17), (31, 32, 33), (47, 48, 49), (63, 64, 65), (129, 249)]
T_ALL = [t for cls in T_CLASSES for t in cls]
HEAD_WIDTHS = [36, 16, 32, 64]           # OB_RA_DISPATCH: d = 16, 32, 36, else (64)
BATCHES = [(1, 1), (3, 3), (6, 3)]      # (Bt, P)


class Guarded:
    """n floats followed by 64 sentinel floats."""

    def __init__(self, shape, gpu):
        n = 1
        for s in shape:
            n *= s
        self.buf = torch.empty(n + N_GUARD, device=gpu)
        self.buf[n:] = SENT
        self.t = self.buf[:n].view(*shape)
        self.n = n

    def nan(self):
        self.t.fill_(float("nan"))

    def intact(self):
        return bool((self.buf[self.n:] == SENT).all().item())


@pytest.fixture(scope="module")
def lib(gpu):
    from onebit_asr import _lib

    lib = _lib.load()
    prev_mode = lib.ob_relattn_set_bwd_mode(0)  # the probability path holds the key-side kernel
    prev_ring = lib.ob_relattn_set_kv_ring(-1)
    assert prev_ring == 1, "the ring is the default"
    yield lib
    lib.ob_relattn_set_bwd_mode(prev_mode)
    lib.ob_relattn_set_kv_ring(prev_ring)


def _lens(bt, t, ragged):
    if not ragged:
        return [t] * bt
    return [max(1, x) for x in (1, t, (t + 1) // 2, t - 1, 1, t)][:bt]


def _run(lib, gpu, bt, P, t, H, d, p, ragged):
    """fwd once; bwd off, on, on from the same saved state. Returns the three output sets."""
    from onebit_asr import _lib

    c = H * d
    g = torch.Generator(device=gpu).manual_seed(1000 * t + 10 * d + bt)
    mk = lambda *s: torch.randn(*s, device=gpu, generator=g)  # noqa: E731
    q, k, v, do = mk(bt, t, c), mk(bt, t, c), mk(bt, t, c), mk(bt, t, c)
    pos, u, vb = mk(P, t, c), mk(H, d) * 0.1, mk(H, d) * 0.1
    lens = torch.tensor(_lens(bt, t, ragged), dtype=torch.int32, device=gpu)
    rng = torch.tensor([1234, 1], dtype=torch.int64, device=gpu)
    n_saved = lib.ob_relattn_saved_elems(bt, t, H, d)
    saved = torch.full((n_saved,), float("nan"), device=gpu)
    ctx = torch.full_like(q, float("nan"))
    s = _lib.stream_of(q)
    _lib.check(lib.ob_relattn_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), pos.data_ptr(),
                                  u.data_ptr(), vb.data_ptr(), lens.data_ptr(), bt, P, t, H, d, p,
                                  rng.data_ptr(), 0, saved.data_ptr(), None, ctx.data_ptr(), s),
               "ob_relattn_fwd")
    wsb = lib.ob_relattn_bwd_workspace(bt, t, H, d)
    ws = torch.empty(wsb + 256, dtype=torch.uint8, device=gpu)
    outs = {n: Guarded(sh, gpu) for n, sh in (("dq", (bt, t, c)), ("dk", (bt, t, c)),
                                               ("dv", (bt, t, c)), ("dpos", (P, t, c)),
                                               ("du", (H, d)), ("dvb", (H, d)))}
    where = f"Bt {bt} P {P} T {t} H {H} d {d} p {p} lens {lens.tolist()}"
    runs = []
    for on in (0, 1, 1):
        for o in outs.values():
            o.nan()
        ws[:wsb] = 0xFF  # NaN as float
        ws[wsb:] = 0xA5
        lib.ob_relattn_set_kv_ring(on)
        _lib.check(lib.ob_relattn_bwd(do.data_ptr(), ctx.data_ptr(), q.data_ptr(), k.data_ptr(),
                                      v.data_ptr(), pos.data_ptr(), u.data_ptr(), vb.data_ptr(),
                                      lens.data_ptr(), bt, P, t, H, d, p, rng.data_ptr(), 0,
                                      saved.data_ptr(), n_saved,
                                      *(outs[n].buf.data_ptr() for n in ("dq", "dk", "dv", "dpos",
                                                                        "du", "dvb")),
                                      ws.data_ptr(), wsb, s), "ob_relattn_bwd")
        for n, o in outs.items():
            assert o.intact(), f"{where}: ring {on}: the sentinel after {n} was overwritten"
        assert bool((ws[wsb:] == 0xA5).all().item()), f"{where}: ring {on}: workspace guard"
        runs.append({n: o.t.clone() for n, o in outs.items()})
    return runs, where


@pytest.mark.parametrize("d", HEAD_WIDTHS)
@pytest.mark.parametrize("t", T_ALL)
def test_kv_ring_same_bits_as_the_two_barrier_kernel(lib, gpu, t, d):
    for bt, P in BATCHES:
        for H in (1, 4):
            for p in (0.0, 0.1):
                for ragged in (False, True):
                    (off, on, on2), where = _run(lib, gpu, bt, P, t, H, d, p, ragged)
                    for n in ("dk", "dv", "dpos", "dq", "du", "dvb"):
                        assert torch.equal(off[n], on[n]), (
                            f"{where}: {n} ring off vs on: "
                            f"{int((off[n] != on[n]).sum())} of {on[n].numel()} elements differ")
                        assert torch.equal(off[n].view(torch.int32), on[n].view(torch.int32)), \
                            f"{where}: {n} ring off vs on differ in a zero's sign"
                        assert torch.equal(on[n], on2[n]), f"{where}: {n} differs between two ring runs"


@pytest.mark.parametrize("t", [cls[-1] for cls in T_CLASSES])
def test_kv_ring_matches_float64(lib, gpu, t):
    """One case per T class (its largest T), d = 36, dropout 0.1, ragged lengths, three passes."""
    from onebit_asr import attention as at

    bt, P, H, d, p = 3, 3, 4, 36, 0.1
    assert lib.ob_relattn_set_kv_ring(1) in (0, 1) and lib.ob_relattn_set_kv_ring(-1) == 1
    q, k, v, pos, u, vb = R.inputs(bt, P, t, H, d, seed=bt * 1000 + t)
    lens_t = torch.tensor(_lens(bt, t, True))
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
    for name, a, b in zip(("dq", "dk", "dv", "dpos", "du", "dvb"), dev, ref_in):
        R.close(a.grad, b.grad, R.GRAD_BAR, f"T {t} {name}")


def test_kv_ring_switch(lib):
    """Returns the previous value; 0 / 1 set it, anything else only queries; on by default
    (the module fixture restores what it found)."""
    start = lib.ob_relattn_set_kv_ring(-1)
    try:
        assert lib.ob_relattn_set_kv_ring(0) == start
        assert lib.ob_relattn_set_kv_ring(7) == 0 and lib.ob_relattn_set_kv_ring(-1) == 0
        assert lib.ob_relattn_set_kv_ring(1) == 0 and lib.ob_relattn_set_kv_ring(-1) == 1
    finally:
        lib.ob_relattn_set_kv_ring(start)
