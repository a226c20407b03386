"""GPU: the minimum-WER loss over the CTC n-best (onebit_asr/mwer.py, csrc/ctcnbest.hip)
against tests/mwer_ref.py (float64 torch on the CPU, gradient by autograd).

Bars (tests/test_ctc_gpu.py's own): loss |out - ref| <= 1e-5 |ref| + 1e-6; gradient max error
<= max(2e-5 max|ref grad|, 2 err32) + 1e-7 with err32 the same composite evaluated by torch in
fp32 against the float64 one; ll 1e-5 relative per live entry. For every case the gradient is
exactly 0.0 outside blank and the n-best's tokens and on padded frames, has no NaN, and a second
call gives the same bits. The shapes are the smallest at which each path runs: the scalar and
the float4 row paths, an adjacent repeat, shared labels, an empty, an absent and an unalignable
entry, an utterance without frames, more states than threads (the strided loops), N = 32, and
one workload-class shape."""
import math

import pytest
import torch

import mwer_ref

pytestmark = pytest.mark.gpu

BLANK = 3
SMALL = [[[5, 5, 7], [5, 7], [], [7, 8, 5, 9]], [[5, 6], [6], [4, 4, 5, 6, 7]]]


def _nbest(ents, N, Th):
    B = len(ents)
    hyp = torch.full((B, N, Th), -1, dtype=torch.int32)
    hyp_len = torch.zeros(B, N, dtype=torch.int32)
    n_hyp = torch.tensor([len(e) for e in ents], dtype=torch.int32)
    for b, es in enumerate(ents):
        for k, e in enumerate(es):
            hyp[b, k, :len(e)] = torch.tensor(e, dtype=torch.int32)
            hyp_len[b, k] = len(e)
    return hyp, hyp_len, n_hyp


def _edits(base, V, n, g, max_len):
    """n entries around ``base``: a few substitutions, deletions and insertions each."""
    out = []
    for k in range(n):
        e = list(base)
        for _ in range(int(torch.randint(0, 4, (1,), generator=g))):
            op = int(torch.randint(0, 3, (1,), generator=g))
            pos = int(torch.randint(0, max(len(e), 1), (1,), generator=g))
            tok = int(torch.randint(4, V, (1,), generator=g))
            if op == 0 and e:
                e[pos] = tok
            elif op == 1 and e:
                del e[pos]
            elif len(e) < max_len:
                e.insert(pos, tok)
        out.append(e)
    return out


def _make(name):
    """-> dict(logits fp32 [B, T, V], lens, hyp, hyp_len, n_hyp, ref, ref_len, scale)."""
    g = torch.Generator().manual_seed(11)
    if name in ("scalar", "float4", "unalignable", "noframes"):
        V = 20 if name == "float4" else 11
        ents = [list(map(list, u)) for u in SMALL]
        lens = [12, 9]
        refs = [[5, 7, 9], [4, 5, 6, 7]]
        if name == "unalignable":  # [4, 4, 5, 6, 7] needs 6 frames
            lens = [12, 5]
        if name == "noframes":
            ents.insert(1, [[5], [], [6, 7]])
            lens = [12, 0, 9]
            refs.insert(1, [5, 6])
        T, N, Th, scale, amp = 12, 4, 5, 0.7, 2.0
    elif name == "strided":  # 2 * 130 + 1 = 261 states > 256 threads
        V, T, N, Th, scale, amp = 12, 300, 2, 130, 0.2, 1.0
        base = [int(v) for v in torch.randint(4, V, (130,), generator=g)]
        ents = [[base, _edits(base[:120], V, 1, g, Th)[0]]]
        lens, refs = [300], [base[:125]]
    elif name == "n32":
        V, T, N, Th, scale, amp = 16, 40, 32, 6, 0.5, 1.5
        base = [5, 9, 9, 12, 7]
        ents = [[base, []] + _edits(base, V, 30, g, Th)]
        lens, refs = [40], [base]
    elif name == "workload":
        V, T, N, Th, scale, amp = 5004, 249, 8, 40, 0.3, 2.0
        ents, refs = [], []
        for L in (40, 27):
            base = [int(v) for v in torch.randint(4, V, (L,), generator=g)]
            ents.append([base] + _edits(base, V, 7, g, Th))
            refs.append(base)
        lens = [249, 200]
    else:
        raise KeyError(name)
    B = len(ents)
    logits = torch.randn(B, T, V, generator=g) * amp
    # the entries' tokens are likelier than the rest, as a trained head's are
    for b, es in enumerate(ents):
        for e in es[:1]:
            for u, v in enumerate(e):
                lo = (u * lens[b]) // max(len(e), 1)
                logits[b, lo:lo + max(lens[b] // max(len(e), 1), 1), v] += 2.0
    hyp, hyp_len, n_hyp = _nbest(ents, N, Th)
    S = max(len(r) for r in refs)
    ref = torch.zeros(B, S, dtype=torch.int64)
    for b, r in enumerate(refs):
        ref[b, :len(r)] = torch.tensor(r)
    return dict(logits=logits, lens=torch.tensor(lens), hyp=hyp, hyp_len=hyp_len, n_hyp=n_hyp,
                ref=ref, ref_len=torch.tensor([len(r) for r in refs]), scale=scale)


_CACHE = {}


def _case(name):
    """The case and its float64 / fp32 CPU references, computed once and left unchanged."""
    if name in _CACHE:
        return _CACHE[name]
    c = _make(name)
    nb = (c["hyp"], c["hyp_len"], c["n_hyp"])
    c["err"] = mwer_ref.token_errors(*nb, c["ref"], c["ref_len"])
    x64 = c["logits"].double().requires_grad_()
    loss, info = mwer_ref.mwer_loss(x64, c["lens"], *nb, c["err"], BLANK, c["scale"])
    c["grad64"] = torch.autograd.grad(loss, x64)[0] if loss.requires_grad \
        else torch.zeros_like(x64)
    c["loss64"], c["ll64"], c["post64"], c["risk64"] = (loss.detach(), info["ll"], info["post"],
                                                        info["risk"])
    x32 = c["logits"].clone().requires_grad_()
    l32, _ = mwer_ref.mwer_loss(x32, c["lens"], *nb, c["err"], BLANK, c["scale"])
    g32 = torch.autograd.grad(l32, x32)[0] if l32.requires_grad else torch.zeros_like(x32)
    c["err32"] = (g32.double() - c["grad64"]).abs().max().item()
    # a general upstream gradient of ll (sum != 0): the dense path's reference
    gw = torch.Generator().manual_seed(3)
    c["w"] = torch.randn(c["ll64"].shape, generator=gw, dtype=torch.float64) + 0.5
    fin = torch.isfinite(c["ll64"])

    def weighted(x):
        ll = mwer_ref.nbest_ll(x, c["lens"], *nb, BLANK)
        return (ll[fin] * c["w"][fin].to(x.dtype)).sum()
    x64 = c["logits"].double().requires_grad_()
    c["wgrad64"] = torch.autograd.grad(weighted(x64), x64)[0] if fin.any() \
        else torch.zeros_like(x64)
    x32 = c["logits"].clone().requires_grad_()
    wg32 = torch.autograd.grad(weighted(x32), x32)[0] if fin.any() else torch.zeros_like(x32)
    c["werr32"] = (wg32.double() - c["wgrad64"]).abs().max().item()
    c["cols"] = mwer_ref.label_columns(*nb, BLANK, c["logits"].shape[2])
    _CACHE[name] = c
    return c


def _run(c, gpu, **kw):
    from onebit_asr.mwer import mwer_ctc_loss

    x = c["logits"].to(gpu).requires_grad_()
    loss, info = mwer_ctc_loss(x, c["lens"].to(gpu), c["ref"].to(gpu), c["ref_len"].to(gpu),
                               c["hyp"].to(gpu), c["hyp_len"].to(gpu), c["n_hyp"].to(gpu),
                               blank_id=BLANK, scale=c["scale"], **kw)
    loss.backward()
    return loss.detach(), info, x.grad


def _check_sparse(c, grad):
    """exactly 0.0 outside blank and the labels, and on padded frames; no NaN."""
    g = grad.cpu()
    assert not torch.isnan(g).any()
    off = g[~c["cols"].unsqueeze(1).expand_as(g)]
    assert torch.equal(off, torch.zeros_like(off))
    for b, tb in enumerate(c["lens"].tolist()):
        assert torch.equal(g[b, tb:], torch.zeros_like(g[b, tb:]))


CASES = ["scalar", "float4", "unalignable", "noframes", "strided", "n32", "workload"]


@pytest.mark.parametrize("name", CASES)
def test_mwer_matches_float64_reference(gpu, name):
    c = _case(name)
    loss, info, grad = _run(c, gpu)
    ref = c["loss64"].item()
    gmax = c["grad64"].abs().max().item()
    err = (grad.cpu().double() - c["grad64"]).abs().max().item()
    ll, ll64 = info["ll"].cpu(), c["ll64"]
    fin = torch.isfinite(ll64)
    llerr = ((ll[fin] - ll64[fin]).abs() / ll64[fin].abs()).max().item() if fin.any() else 0.0
    print(f"{name}: loss {loss.item():.7f} ref {ref:.7f}; grad err {err:.3e} of max {gmax:.3e} "
          f"(fp32 torch: {c['err32']:.3e}); ll rel err {llerr:.3e}")
    assert loss.dtype == torch.float32 and ll.dtype == torch.float64
    assert torch.equal(torch.isfinite(ll), fin) and (ll[~fin] == -math.inf).all()
    assert llerr <= 1e-5
    assert abs(loss.item() - ref) <= 1e-5 * abs(ref) + 1e-6, (loss.item(), ref)
    assert err <= max(2e-5 * gmax, 2 * c["err32"]) + 1e-7, (err, c["err32"])
    torch.testing.assert_close(info["post"].cpu(), c["post64"], rtol=1e-3, atol=1e-5)
    torch.testing.assert_close(info["risk"].cpu(), c["risk64"], rtol=1e-3, atol=1e-5)
    assert torch.equal(info["err"].cpu()[fin], c["err"][fin])  # ob_nbest_edit_distance's dref
    _check_sparse(c, grad)
    assert gmax > 1e-4  # the case exercises the gradient
    loss2, info2, grad2 = _run(c, gpu)
    assert torch.equal(loss, loss2) and torch.equal(grad, grad2)
    assert torch.equal(info["ll"], info2["ll"])
    for k in ("ll", "post", "err", "risk", "hyp", "hyp_len", "n_hyp"):
        assert not info[k].requires_grad


@pytest.mark.parametrize("name", CASES)
def test_nbest_logprob_dense_gradient(gpu, name):
    """nbest_ctc_logprob under upstream weights whose sum is not zero: the softmax term is
    written too. The same bars."""
    from onebit_asr.mwer import nbest_ctc_logprob

    c = _case(name)
    fin = torch.isfinite(c["ll64"])
    x = c["logits"].to(gpu).requires_grad_()
    nb = [c[k].to(gpu) for k in ("hyp", "hyp_len", "n_hyp")]
    ll = nbest_ctc_logprob(x, c["lens"].to(gpu), *nb, blank_id=BLANK)
    assert ll.dtype == torch.float64 and ll.shape == c["ll64"].shape
    (ll[fin.to(gpu)] * c["w"].to(gpu)[fin.to(gpu)]).sum().backward()
    gmax = c["wgrad64"].abs().max().item()
    err = (x.grad.cpu().double() - c["wgrad64"]).abs().max().item()
    print(f"{name}: dense grad err {err:.3e} of max {gmax:.3e} (fp32 torch: {c['werr32']:.3e})")
    assert not torch.isnan(x.grad).any()
    assert err <= max(2e-5 * gmax, 2 * c["werr32"]) + 1e-7, (err, c["werr32"])
    for b, tb in enumerate(c["lens"].tolist()):
        assert not x.grad[b, tb:].any()
    g1 = x.grad.clone()
    x.grad = None
    ll2 = nbest_ctc_logprob(x, c["lens"].to(gpu), *nb, blank_id=BLANK)
    (ll2[fin.to(gpu)] * c["w"].to(gpu)[fin.to(gpu)]).sum().backward()
    assert torch.equal(ll, ll2) and torch.equal(g1, x.grad)


@pytest.mark.parametrize("name", ["scalar", "float4", "workload"])
def test_batch_slot_does_not_change_the_bits(gpu, name):
    """The same utterance in batch slot 0 and in slot 1: the same ll and gradient bits."""
    c = _case(name)
    swapped = dict(c)
    for k in ("logits", "lens", "hyp", "hyp_len", "n_hyp", "ref", "ref_len"):
        swapped[k] = c[k][[1, 0]].contiguous()
    _, info_a, grad_a = _run(c, gpu)
    _, info_b, grad_b = _run(swapped, gpu)
    assert torch.equal(info_a["ll"], info_b["ll"][[1, 0]])
    assert torch.equal(info_a["post"], info_b["post"][[1, 0]])
    assert torch.equal(grad_a, grad_b[[1, 0]])


def test_single_entry_equals_the_training_ctc(gpu):
    """N = 1 and hyp = ref: mean(-ll / max(L, 1)) is ctc_loss_logits_groups' loss."""
    from onebit_asr.ctc import ctc_loss_logits_groups
    from onebit_asr.mwer import nbest_ctc_logprob

    g = torch.Generator().manual_seed(2)
    B, T, V, S = 3, 40, 20, 8
    x = (torch.randn(B, T, V, generator=g) * 2).to(gpu)
    tg = torch.randint(4, V, (B, S), generator=g)
    tg[1, 1] = tg[1, 0]  # an adjacent repeat
    il, tl = torch.tensor([40, 33, 20]), torch.tensor([8, 5, 0])
    want = ctc_loss_logits_groups(x, tg.to(gpu), il.to(gpu), tl.to(gpu), BLANK, 1)[0]
    ll = nbest_ctc_logprob(x, il.to(gpu), tg.to(gpu).unsqueeze(1), tl.to(gpu).unsqueeze(1),
                           torch.ones(B, dtype=torch.int32, device=gpu), blank_id=BLANK)
    got = (-ll[:, 0] / tl.to(gpu).clamp(min=1)).mean()
    assert torch.allclose(got.float(), want, rtol=1e-6, atol=0), (got, want)


def test_internal_search_and_supplied_errors(gpu):
    """hyp=None: the n-best is ctc_beam_search_nbest_device's on the same logits; errors=: the
    loss follows the supplied counts."""
    from onebit_asr.infer import ctc_beam_search_nbest_device
    from onebit_asr.mwer import mwer_ctc_loss

    c = _case("float4")
    x = c["logits"].to(gpu).requires_grad_()
    lens, ref, ref_len = c["lens"].to(gpu), c["ref"].to(gpu), c["ref_len"].to(gpu)
    loss, info = mwer_ctc_loss(x, lens, ref, ref_len, beam_size=6, nbest=4, blank_id=BLANK)
    hyp, hyp_len, n_hyp, _ = ctc_beam_search_nbest_device(x.detach(), lens, beam_size=6, nbest=4,
                                                          blank_id=BLANK)
    assert torch.equal(info["hyp"], hyp) and torch.equal(info["hyp_len"], hyp_len)
    assert torch.equal(info["n_hyp"], n_hyp) and int(n_hyp.min()) >= 2
    loss.backward()
    assert torch.isfinite(x.grad).all()
    # against the reference on that n-best
    nb = (hyp.cpu(), hyp_len.cpu(), n_hyp.cpu())
    err = mwer_ref.token_errors(*nb, c["ref"], c["ref_len"])
    want, _ = mwer_ref.mwer_loss(c["logits"].double(), c["lens"], *nb, err, BLANK, 1.0)
    assert abs(loss.item() - want.item()) <= 1e-5 * abs(want.item()) + 1e-6
    # supplied counts (word-level ones, say): the loss follows them
    mine = torch.arange(8, dtype=torch.float64).reshape(2, 4) * 1.5
    loss_e, info_e = mwer_ctc_loss(x, lens, None, None, hyp, hyp_len, n_hyp, blank_id=BLANK,
                                   scale=0.5, errors=mine.to(gpu))
    want_e, _ = mwer_ref.mwer_loss(c["logits"].double(), c["lens"], *nb, mine, BLANK, 0.5)
    assert torch.equal(info_e["err"].cpu(), mine)
    assert abs(loss_e.item() - want_e.item()) <= 1e-5 * abs(want_e.item()) + 1e-6
    assert abs(loss_e.item() - loss.item()) > 1e-3


def test_capture_and_replay(gpu):
    """Forward + backward, the internal beam search included, captured in a HIP graph and
    replayed on refreshed logits: the eager call's loss and gradient bits."""
    from onebit_asr.mwer import mwer_ctc_loss

    c = _case("float4")
    lens, ref, ref_len = c["lens"].to(gpu), c["ref"].to(gpu), c["ref_len"].to(gpu)
    x = c["logits"].to(gpu).requires_grad_()

    def fwd_bwd():
        loss, info = mwer_ctc_loss(x, lens, ref, ref_len, beam_size=6, nbest=4, blank_id=BLANK)
        return loss.detach(), torch.autograd.grad(loss, x)[0], info["hyp_len"]

    side = torch.cuda.Stream(gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        fwd_bwd()
    torch.cuda.current_stream(gpu).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fwd_bwd()
    fresh = torch.randn(c["logits"].shape, generator=torch.Generator().manual_seed(77)) * 2
    for logits in (fresh, c["logits"]):
        with torch.no_grad():
            x.copy_(logits.to(gpu))
        graph.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in out]
        want = fwd_bwd()
        torch.cuda.synchronize()
        for a, b in zip(got, want):
            assert torch.equal(a, b)
        assert got[1].abs().max().item() > 0


def _model_and_batch(gpu, seed=1234):
    """tests/test_graph_step_gpu.py's model and batch. An untrained head's n-best is the empty
    entry and single wrong tokens, all at the same distance from the reference (a zero loss and
    gradient), so the head's bias favours blank and the first reference's first tokens: the
    entries then differ in their error counts."""
    from _steputil import build
    from onebit_asr.data import CFG1, synthetic_batch

    model = build(CFG1, gpu, seed=seed)
    batch = synthetic_batch([734, 349], [27, 12], seed=0, device=gpu)
    with torch.no_grad():
        model.ctc_head.bias[batch["tokens"][0, :3]] += 4.0
        model.ctc_head.bias[BLANK] += 5.0
    return model, batch


def _step_once(gpu, **kw):
    from _steputil import grads
    from onebit_asr.train_step import OneBitStep

    model, batch = _model_and_batch(gpu)
    step = OneBitStep(model, n_layers=2, **kw)
    bits = step.make_bits(gpu)
    bits.set([1, 0])
    loss, parts = step(batch, bits)
    loss.backward()
    torch.cuda.synchronize()
    return step, loss.detach().clone(), parts.clone(), grads(model)


def test_step_with_mwer_weight(gpu):
    """mwer_weight = 0 is today's step bit for bit; 0.5 adds 0.5 * last_mwer and reaches the
    CTC head."""
    _, l0, p0, g0 = _step_once(gpu)
    step_z, lz, pz, gz = _step_once(gpu, mwer_weight=0.0)
    assert step_z.last_mwer is None
    assert torch.equal(l0, lz) and torch.equal(p0, pz)
    for k in g0:
        assert (g0[k] is None) == (gz[k] is None), k
        assert g0[k] is None or torch.equal(g0[k], gz[k]), k
    step_m, lm, pm, gm = _step_once(gpu, mwer_weight=0.5)
    mw = step_m.last_mwer
    assert mw.is_cuda and mw.dim() == 0 and not mw.requires_grad and torch.isfinite(mw)
    assert mw.item() != 0.0
    assert pm.shape == (8,) and torch.equal(pm, p0)
    print(f"step loss {l0.item():.6f} + 0.5 * mwer {mw.item():.6f} = {lm.item():.6f}")
    want = l0.item() + 0.5 * mw.item()
    assert abs(lm.item() - want) <= 4e-7 * (abs(l0.item()) + abs(0.5 * mw.item())), (lm, want)
    for k, g in gm.items():
        assert g is None or torch.isfinite(g).all(), k
    assert not torch.equal(gm["ctc_head.weight"], g0["ctc_head.weight"])


def test_step_with_mwer_under_graphed_train_step(gpu):
    """GraphedTrainStep with the MWER term: graph replay == the same class run eagerly."""
    from onebit_asr.graph_step import GraphedTrainStep
    from onebit_asr.train_step import OneBitStep

    out = {}
    for use_graph in (True, False):
        model, batch = _model_and_batch(gpu, seed=0)
        step = OneBitStep(model, n_layers=2, mwer_weight=0.5)
        gs = GraphedTrainStep(step, n_layers=2, warmup_iters=2, warmup_steps=4, total_steps=20,
                              use_graph=use_graph)
        res = []
        for mask in ([1, 0], [0, 1]):
            loss, _ = gs.step(batch, mask)
            res.append((loss.item(), step.last_mwer.item()))
        assert (gs.graph_a is not None) == use_graph
        out[use_graph] = res
    print(out)
    for res in out.values():
        assert all(math.isfinite(v) for pair in res for v in pair)
        assert res[0] != res[1]  # the second step (new mask, updated weights) took effect
    # the first step starts from the same weights on both sides; after an update the n-best, a
    # discrete choice, may differ between weights that differ by rounding
    (lg, mg), (le, me) = out[True][0], out[False][0]
    assert abs(lg - le) <= 1e-5 * abs(le) and abs(mg - me) <= 1e-5 * abs(me) + 1e-6
