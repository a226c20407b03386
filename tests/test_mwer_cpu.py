"""CPU: the reference of the minimum-WER loss (tests/mwer_ref.py) on a hand-derived case, the
cancellation that makes its gradient sparse, the single-live-entry rule; the argument validation
of the new C entries (before any HIP call) and the Python surface."""
import inspect
import math

import pytest
import torch

import mwer_ref
import onebit_asr.mwer as mwer_mod

OK, NULL, SHAPE, WS, ALIGN = 0, -1, -2, -4, -5


def _nbest(ents, N, Th):
    """entries per utterance -> (hyp [B, N, Th] padded with -1, hyp_len [B, N], n_hyp [B])."""
    B = len(ents)
    hyp = torch.full((B, N, Th), -1, dtype=torch.int32)
    hyp_len = torch.zeros(B, N, dtype=torch.int32)
    n_hyp = torch.tensor([len(e) for e in ents], dtype=torch.int32)
    for b, es in enumerate(ents):
        for k, e in enumerate(es):
            hyp[b, k, :len(e)] = torch.tensor(e, dtype=torch.int32)
            hyp_len[b, k] = len(e)
    return hyp, hyp_len, n_hyp


@pytest.mark.parametrize("scale", [1.0, 0.5, 2.0])
def test_hand_derived_known_answer(scale):
    """V = 3 uniform logits, T = 2, blank 0, entries [a] and [], reference [a]. Every path has
    probability 1/9; [a] has the three paths a-, -a, aa and [] the one path --: ll = (log 1/3,
    log 1/9), post = 3^s : 1, err = (0, 1), base = 1/2."""
    logits = torch.zeros(1, 2, 3, dtype=torch.float64, requires_grad=True)
    hyp, hyp_len, n_hyp = _nbest([[[1], []]], 2, 1)
    ref, ref_len = torch.tensor([[1]]), torch.tensor([1])
    err = mwer_ref.token_errors(hyp, hyp_len, n_hyp, ref, ref_len)
    assert err.tolist() == [[0.0, 1.0]]
    loss, info = mwer_ref.mwer_loss(logits, torch.tensor([2]), hyp, hyp_len, n_hyp, err, 0, scale)
    want_ll = torch.tensor([[math.log(1 / 3), math.log(1 / 9)]], dtype=torch.float64)
    torch.testing.assert_close(info["ll"], want_ll, rtol=1e-14, atol=0)
    p1 = 1.0 / (3.0 ** scale + 1.0)  # the posterior of the empty entry = the risk
    torch.testing.assert_close(info["post"], torch.tensor([[1 - p1, p1]], dtype=torch.float64),
                               rtol=1e-13, atol=0)
    assert abs(info["risk"].item() - p1) <= 1e-14
    assert abs(loss.item() - (p1 - 0.5)) <= 1e-14
    if scale == 1.0:
        assert abs(loss.item() + 0.25) <= 1e-14 and abs(info["risk"].item() - 0.25) <= 1e-14


def _small_case(V=11, lens=(12, 9)):
    g = torch.Generator().manual_seed(5)
    logits = torch.randn(2, 12, V, generator=g, dtype=torch.float64) * 2
    ents = [[[5, 5, 7], [5, 7], [], [7, 8, 5, 9]], [[5, 6], [6], [4, 4, 5, 6, 7]]]
    hyp, hyp_len, n_hyp = _nbest(ents, 4, 5)
    ref = torch.tensor([[5, 7, 9, 0], [4, 5, 6, 7]])
    ref_len = torch.tensor([3, 4])
    return logits, torch.tensor(lens), hyp, hyp_len, n_hyp, ref, ref_len


def test_reference_gradient_is_sparse():
    """sum_k dL/dll_k = 0 per utterance, so the softmax terms cancel: outside blank and the
    n-best's tokens the float64 gradient is rounding noise, and exactly 0 on padded frames."""
    logits, lens, hyp, hyp_len, n_hyp, ref, ref_len = _small_case()
    x = logits.clone().requires_grad_()
    err = mwer_ref.token_errors(hyp, hyp_len, n_hyp, ref, ref_len)
    loss, info = mwer_ref.mwer_loss(x, lens, hyp, hyp_len, n_hyp, err, 3, 0.7)
    loss.backward()
    cols = mwer_ref.label_columns(hyp, hyp_len, n_hyp, 3, logits.shape[2])
    off = x.grad[~cols.unsqueeze(1).expand_as(x.grad)]
    print(f"loss {loss.item():.6f}; max |grad| {x.grad.abs().max().item():.3e}; outside the "
          f"label columns {off.abs().max().item():.3e}")
    assert x.grad.abs().max().item() > 1e-3  # the case is not degenerate
    assert off.abs().max().item() < 1e-12
    assert torch.equal(x.grad[1, 9:], torch.zeros_like(x.grad[1, 9:]))


def test_single_live_entry_gives_zero():
    """lens = 5: [4, 4, 5, 6, 7] needs 6 frames and is not live; with n_hyp = 1, or with every
    other entry unalignable, the utterance has one live entry: loss 0, gradient 0."""
    logits, _, hyp, hyp_len, n_hyp, ref, ref_len = _small_case()
    err = mwer_ref.token_errors(hyp, hyp_len, n_hyp, ref, ref_len)
    lens = torch.tensor([12, 5])
    ll = mwer_ref.nbest_ll(logits, lens, hyp, hyp_len, n_hyp, 3)
    assert torch.isfinite(ll[1, :2]).all() and ll[1, 2] == -math.inf and ll[1, 3] == -math.inf
    x = logits[1:].clone().requires_grad_()
    loss, info = mwer_ref.mwer_loss(x, torch.tensor([1]), hyp[1:], hyp_len[1:], n_hyp[1:],
                                    err[1:], 3, 1.0)  # one frame: only [6] aligns
    assert torch.isfinite(info["ll"][0]).tolist() == [False, True, False, False]
    loss.backward() if loss.requires_grad else None
    assert loss.item() == 0.0
    assert x.grad is None or not x.grad.any()
    assert info["post"][0].tolist() == [0.0, 1.0, 0.0, 0.0] and info["risk"][0] == err[1, 1]


def test_new_entries_validate_before_any_hip_call():
    """Every check below fails before any HIP call, so it is safe with no device."""
    from onebit_asr import _lib

    lib = _lib.load()
    sup = lib.ob_ctc_nbest_supported
    assert sup(1, 0) == 1 and sup(32, 511) == 1 and sup(mwer_mod.MAX_NBEST, mwer_mod.MAX_LEN) == 1
    assert sup(33, 5) == 0 and sup(4, 512) == 0 and sup(0, 5) == 0 and sup(4, -1) == 0
    ws = lib.ob_ctc_nbest_workspace
    assert ws(2, 33, 12, 5) == 0 and ws(2, 4, 12, 512) == 0 and ws(0, 4, 12, 5) == 0
    assert ws(2, 4, 0, 5) == 0 and ws(1 << 20, 32, 1 << 12, 5) == 0
    need = ws(2, 4, 12, 5)
    # at least alpha and beta [B N][T][2 Th + 1] and the compact log-probs [B N T][Th + 1], fp32
    assert need >= 4 * (2 * 8 * 12 * 11 + 8 * 12 * 6) and need % 256 == 0
    print(f"workspace: B=2 N=4 T=12 Th=5: {need} bytes; B=32 N=10 T=249 Th=40: "
          f"{ws(32, 10, 249, 40)} bytes; N=4: {ws(32, 4, 249, 40)} bytes")
    f = 0x3000  # never dereferenced (256-byte aligned)

    # logits, lens, hyp, hyp_len, n_hyp, B, N, T, V, Th, blank, ws, ws_bytes, ll
    def logprob(**kw):
        a = dict(logits=f, lens=f, hyp=f, hyp_len=f, n_hyp=f, B=2, N=4, T=12, V=11, Th=5, blank=3,
                 ws=f, ws_bytes=need - 1, ll=f)
        a.update(kw)
        return lib.ob_ctc_nbest_logprob(*a.values(), None)

    # ..., blank, coef, grad_out, dense, ws, ws_bytes, grad
    def grad(**kw):
        a = dict(logits=f, lens=f, hyp=f, hyp_len=f, n_hyp=f, B=2, N=4, T=12, V=11, Th=5, blank=3,
                 coef=f, grad_out=f, dense=0, ws=f, ws_bytes=need - 1, grad=f)
        a.update(kw)
        return lib.ob_ctc_nbest_grad(*a.values(), None)

    for call, out in ((logprob, "ll"), (grad, "grad")):
        assert call() == WS                      # one byte short, everything else valid
        assert call(N=33) == SHAPE and call(Th=512) == SHAPE and call(N=0) == SHAPE
        assert call(B=0) == SHAPE and call(T=0) == SHAPE and call(V=0) == SHAPE
        assert call(blank=11) == SHAPE and call(blank=-1) == SHAPE and call(Th=-1) == SHAPE
        for name in ("logits", "lens", "hyp", "hyp_len", "n_hyp", "ws", out):
            assert call(**{name: None}) == NULL, name
        for name in ("logits", "hyp", "hyp_len", "n_hyp", out):
            assert call(**{name: 0x3002}) == ALIGN, name
        assert call(lens=0x3004) == ALIGN and call(ws=0x3008) == ALIGN
        assert call(V=12, logits=0x3004) == ALIGN  # the float4 row path
        assert call(Th=0, hyp=None, ws_bytes=ws(2, 4, 12, 0) - 1) == WS  # no tokens, no array
    assert grad(coef=None) == NULL and grad(grad_out=None) == WS  # the upstream gradient: 1
    assert grad(coef=0x3004) == ALIGN and grad(V=12, grad=0x3004) == ALIGN

    # ll, err, n_hyp, scale, B, N, loss, post, risk, coef
    def combine(**kw):
        a = dict(ll=f, err=f, n_hyp=f, scale=1.0, B=2, N=4, loss=f, post=f, risk=f, coef=f)
        a.update(kw)
        return lib.ob_mwer_combine(*a.values(), None)
    assert combine(N=33) == SHAPE and combine(N=0) == SHAPE and combine(B=0) == SHAPE
    assert combine(scale=-1.0) == SHAPE and combine(scale=math.inf) == SHAPE
    assert combine(scale=math.nan) == SHAPE
    for name in ("ll", "err", "n_hyp", "loss", "post", "risk", "coef"):
        assert combine(**{name: None}) == NULL, name
    for name in ("ll", "err", "loss", "post", "risk", "coef"):
        assert combine(**{name: 0x3004}) == ALIGN, name
    assert combine(n_hyp=0x3002) == ALIGN


def test_python_surface_on_cpu():
    import onebit_asr
    from onebit_asr.train_step import OneBitStep

    assert onebit_asr.mwer_ctc_loss is mwer_mod.mwer_ctc_loss
    assert onebit_asr.nbest_ctc_logprob is mwer_mod.nbest_ctc_logprob
    sig = inspect.signature(mwer_mod.mwer_ctc_loss)
    assert list(sig.parameters) == ["logits", "lens", "ref", "ref_len", "hyp", "hyp_len", "n_hyp",
                                    "beam_size", "nbest", "top_k_per_t", "blank_id", "scale",
                                    "errors"]
    d = {k: p.default for k, p in sig.parameters.items()}
    assert (d["beam_size"], d["nbest"], d["top_k_per_t"], d["blank_id"], d["scale"]) == \
        (10, 4, 20, 3, 1.0)
    assert sig.parameters["beam_size"].kind is inspect.Parameter.KEYWORD_ONLY
    assert inspect.signature(mwer_mod.nbest_ctc_logprob).parameters["blank_id"].default == 3
    sd = {k: p.default for k, p in inspect.signature(OneBitStep.__init__).parameters.items()}
    assert (sd["mwer_weight"], sd["mwer_nbest"], sd["mwer_beam"], sd["mwer_scale"]) == \
        (0.0, 4, 8, 1.0)
    logits, lens, hyp, hyp_len, n_hyp, ref, ref_len = _small_case()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mwer_mod.mwer_ctc_loss(logits.float(), lens, ref, ref_len, hyp, hyp_len, n_hyp)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mwer_mod.nbest_ctc_logprob(logits.float(), lens, hyp, hyp_len, n_hyp)
    with pytest.raises(ValueError, match="scale"):
        mwer_mod.mwer_ctc_loss(logits.float(), lens, ref, ref_len, hyp, hyp_len, n_hyp, scale=-1)
    with pytest.raises(ValueError, match="go together"):
        mwer_mod.mwer_ctc_loss(logits.float(), lens, ref, ref_len, hyp, None, n_hyp)
