"""GPU: two-pass decoding -- the CTC n-best (csrc/beam.hip), the grouped decoder attention
(csrc/decattn.hip), the fused sequence scorer and the prepare / select kernels
(csrc/rescore.hip), and ``decoder="rescore"`` end to end, eager and graphed -- against the
float64 oracle of tests/rescore_ref.py.

Bars. N-best scores: 1e-9 * max(1, T), the bar of test_beam_search_gpu.py; hypotheses exact
where the oracle's smallest decision margin (the gaps inside the final ranking included) is
>= 1e-6. Scorer: |lp - ref| <= max(1e-5 * max|logit|, 4 * e_torch) with e_torch the error of
torch's fp32 CPU expression against the same float64 reference (measured per case, printed).
End to end: att within 4x the error the existing path (``model.decode_logits`` on the GPU, then
log_softmax + gather in float64 on the host) shows against the same oracle on the same inputs.

Worst figures seen on an MI355X (each test prints its own, -s): n-best score error 1.4e-14;
scorer error 3.1e-5 at R=64 d=256 V=64 (max|logit| 69.8, e_torch 1.8e-5, bar 7.0e-4) and
2.4e-5 at R=130 d=144 V=5004 (max|logit| 80.5, e_torch 2.0e-5, bar 8.1e-4); end-to-end att
error 6.2e-6 where the existing path shows 2.5e-6 (bar 9.9e-6), the oracle's winner on every
utterance (smallest oracle gap 0.18).
"""
import functools

import numpy as np
import pytest
import torch

import rescore_ref as rr
from ctc_beam_ref import ctc_like_logits, ragged_lens

pytestmark = pytest.mark.gpu

BLANK = 3
MARGIN = 1e-6

#              B   T    V   beam nbest  seed
NBEST_CASES = [(1, 1, 5, 10, 10, 2000),      # fewer live prefixes than nbest
               (3, 17, 7, 10, 10, 2001),
               (4, 64, 40, 4, 4, 2002),
               (4, 64, 40, 10, 3, 2003),
               (2, 16, 5004, 10, 10, 2004),
               (2, 40, 12, 32, 32, 2005)]


@functools.lru_cache(maxsize=None)
def _nbest_case(i):
    B, T, V, beam, nbest, seed = NBEST_CASES[i]
    logits = ctc_like_logits(seed, B, T, V, BLANK)
    lens = ragged_lens(seed, B, T)
    logits.setflags(write=False)
    lens.setflags(write=False)
    return logits, lens, tuple(rr.nbest_search_batch(logits, lens, beam, BLANK, 20))


def _nbest_device(logits, lens, gpu, beam, nbest):
    from onebit_asr.infer import ctc_beam_search_nbest_device

    res = ctc_beam_search_nbest_device(torch.from_numpy(np.ascontiguousarray(logits)).to(gpu),
                                       torch.from_numpy(np.asarray(lens)).to(gpu),
                                       beam_size=beam, nbest=nbest, blank_id=BLANK)
    hyp, hyp_len, n_hyp, score = res
    assert hyp.dtype == hyp_len.dtype == n_hyp.dtype == torch.int32
    assert score.dtype == torch.float64 and all(t.is_cuda for t in res)
    B, T = logits.shape[:2]
    assert hyp.shape == (B, nbest, T) and hyp_len.shape == score.shape == (B, nbest)
    assert n_hyp.shape == (B,)
    return tuple(t.cpu().numpy() for t in res)


def _one_best_device(logits, lens, gpu, beam):
    from onebit_asr.infer import ctc_beam_search_batch_device

    res = ctc_beam_search_batch_device(torch.from_numpy(np.ascontiguousarray(logits)).to(gpu),
                                       torch.from_numpy(np.asarray(lens)).to(gpu),
                                       beam_size=beam, blank_id=BLANK)
    return tuple(t.cpu().numpy() for t in res)


@pytest.mark.parametrize("i", range(len(NBEST_CASES)),
                         ids=["-".join(map(str, c[:5])) for c in NBEST_CASES])
def test_nbest_matches_oracle(gpu, i):
    B, T, V, beam, nbest, _ = NBEST_CASES[i]
    logits, lens, refs = _nbest_case(i)
    assert lens[0] == T and (B == 1 or lens[-1] == 0)
    # the condition on the test itself, from the oracle alone
    assert sum(r.margin < MARGIN for r in refs) <= B // 16
    hyp, hyp_len, n_hyp, score = _nbest_device(logits, lens, gpu, beam, nbest)
    low = 0
    for b, r in enumerate(refs):
        n = min(len(r.hyps), nbest)
        assert n_hyp[b] == n, (b, n_hyp[b], n)
        errs = [abs(score[b, k] - r.scores[k]) for k in range(n)]
        print(f"utt {b}: margin {r.margin:.3e} n_hyp {n} worst score err {max(errs):.3e}")
        assert max(errs) <= 1e-9 * max(1, T)
        got = []
        for k in range(nbest):
            m = int(hyp_len[b, k])
            assert 0 <= m <= T and (hyp[b, k, m:] == -1).all(), (b, k)
            got.append(hyp[b, k, :m].tolist())
            if k >= n:  # absent
                assert m == 0 and score[b, k] == -np.inf
        if r.margin >= MARGIN:
            assert got[:n] == r.hyps[:n], (b, got[:n], r.hyps[:n])
        else:
            low += 1
            assert sorted(got[:n]) == sorted(r.hyps[:n]), b
        if lens[b] == 0:
            assert n == 1 and got[0] == [] and score[b, 0] == 0.0
    assert low <= B // 16
    # entry 0 is the 1-best call, bit for bit; nbest = 1 is that call
    out, cnt, sc1 = _one_best_device(logits, lens, gpu, beam)
    assert (hyp[:, 0, :] == out).all() and (hyp_len[:, 0] == cnt).all()
    assert (score[:, 0].view(np.int64) == sc1.view(np.int64)).all()
    h1, l1, n1, s1 = _nbest_device(logits, lens, gpu, beam, 1)
    assert (h1[:, 0, :] == out).all() and (l1[:, 0] == cnt).all() and (n1 == 1).all()
    assert (s1[:, 0].view(np.int64) == sc1.view(np.int64)).all()
    # run to run
    again = _nbest_device(logits, lens, gpu, beam, nbest)
    for a, b_ in zip((hyp, hyp_len, n_hyp, score), again):
        assert a.tobytes() == b_.tobytes()


# ------------------------------------------------------------------------------------------
# grouped attention
# ------------------------------------------------------------------------------------------
def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("dh", [16, 36])
def test_grouped_attention_is_the_plain_forward_on_repeated_memory(gpu, dh):
    from onebit_asr import _lib

    lib = _lib.load()
    B, G, H = 2, 3, 4
    e = H * dh
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(dh)
    for Lq in (1, 17):
        for Lk in (1, 249, 256):
            assert lib.ob_decattn_supported(Lq, Lk, dh)
            q = torch.randn(B * G, Lq, e, generator=g).to(gpu)
            kv = torch.randn(B, Lk, 2 * e, generator=g).to(gpu)
            kmask = torch.zeros(B, Lk, dtype=torch.bool)
            kmask[0, (2 * Lk + 2) // 3:] = True  # ragged: utterance 0 keeps about two thirds
            kmask = kmask.to(gpu)
            kv_rep = kv.repeat_interleave(G, 0).contiguous()
            km_rep = kmask.repeat_interleave(G, 0).contiguous()
            for causal in (0, 1):
                for group, qq in ((G, q), (1, q[:B].contiguous())):
                    rows = B * group
                    kvr, kmr = (kv_rep, km_rep) if group == G else (kv, kmask)
                    ref = torch.empty(rows, Lq, e, device=gpu)
                    probs = torch.empty(rows, H, Lq, Lk, device=gpu)
                    assert lib.ob_decattn_fwd(qq.data_ptr(), e, kvr.data_ptr(), 2 * e,
                                              kvr.data_ptr() + 4 * e, 2 * e, kmr.data_ptr(), causal,
                                              rows, H, Lq, Lk, dh, 0.0, None, 0, probs.data_ptr(),
                                              ref.data_ptr(), st) == 0
                    got = torch.full((rows, Lq, e), float("nan"), device=gpu)
                    assert lib.ob_decattn_fwd_grouped(qq.data_ptr(), e, kv.data_ptr(), 2 * e,
                                                      kv.data_ptr() + 4 * e, 2 * e,
                                                      kmask.data_ptr(), causal, B, group, H, Lq,
                                                      Lk, dh, got.data_ptr(), st) == 0
                    assert torch.equal(_bits(got), _bits(ref)), (Lq, Lk, causal, group)
                    if not causal or Lq == 1:  # (causal with Lq > Lk masks nothing more here)
                        assert torch.isfinite(got).all()
    # a shape the core does not take
    q = torch.zeros(B * G, 2, e, device=gpu)
    kv = torch.zeros(B, 257, 2 * e, device=gpu)
    out = torch.zeros(B * G, 2, e, device=gpu)
    assert not lib.ob_decattn_supported(2, 257, dh)
    assert lib.ob_decattn_fwd_grouped(q.data_ptr(), e, kv.data_ptr(), 2 * e, kv.data_ptr() + 4 * e,
                                      2 * e, None, 0, B, G, H, 2, 257, dh, out.data_ptr(),
                                      st) == _lib.OB_ERR_SHAPE


def test_python_grouped_attention_matches_dec_attention(gpu):
    from onebit_asr.decattn import dec_attention, dec_attention_grouped

    g = torch.Generator().manual_seed(3)
    q = torch.randn(6, 5, 64, generator=g).to(gpu)
    kv = torch.randn(2, 40, 128, generator=g).to(gpu)
    km = torch.zeros(2, 40, dtype=torch.bool)
    km[1, 25:] = True
    km = km.to(gpu)
    ref = dec_attention(q, kv.repeat_interleave(3, 0), 4, km.repeat_interleave(3, 0), False, 0.1,
                        False)
    got = dec_attention_grouped(q, kv, 4, km, 3)
    assert torch.equal(_bits(got), _bits(ref))


# ------------------------------------------------------------------------------------------
# the fused scorer
# ------------------------------------------------------------------------------------------
#              R    d    V
SCORE_CASES = [(0, 16, 5), (1, 16, 1), (63, 64, 5), (64, 256, 64), (65, 16, 5004),
               (130, 144, 5004)]


@functools.lru_cache(maxsize=None)
def _score_case(i):
    R, d, V = SCORE_CASES[i]
    rng = np.random.default_rng(4000 + i)
    h = rng.standard_normal((R, d)).astype(np.float32)
    W = rng.standard_normal((V, d)).astype(np.float32)
    bias = rng.standard_normal(V).astype(np.float32)
    tgt = rng.integers(0, V, size=R).astype(np.int32)
    if R >= 3 and V > 128:
        # rows whose largest logit (about 80) sits in the first, a middle and the last column
        # tile: h = s * W[c] with s = 80 / |W[c]|^2
        for r, c in ((0, 5), (1, V // 2), (2, V - 3)):
            h[r] = W[c] * np.float32(80.0 / float((W[c].astype(np.float64) ** 2).sum()))
    if R >= 8:
        tgt[3] = 0            # column 0
        tgt[4] = V - 1        # the last column
        tgt[5] = V - 1 - (V - 1) % 64 + ((V - 1) % 64) // 2  # inside the tail tile
        tgt[6] = -1           # skipped rows mixed in
        tgt[R - 1] = -1 if R % 2 else tgt[R - 1]
    if R >= 130:
        tgt[64:128] = -1      # an all-skip 64-row stretch (four whole subtiles)
    ref, mx = rr.seq_logprob(h, W, bias, tgt.tolist())
    th, tW, tb = torch.from_numpy(h), torch.from_numpy(W), torch.from_numpy(bias)
    lsm = torch.log_softmax(torch.nn.functional.linear(th, tW, tb), dim=-1).numpy()
    live = tgt >= 0
    e_torch = float(np.abs(lsm[np.arange(R)[live], tgt[live]] - ref[live]).max()) if live.any() else 0.0
    for a in (h, W, bias, tgt, ref):
        a.setflags(write=False)
    return h, W, bias, tgt, ref, mx, e_torch


@pytest.mark.parametrize("i", range(len(SCORE_CASES)),
                         ids=["x".join(map(str, c)) for c in SCORE_CASES])
def test_scorer_matches_float64(gpu, i):
    from onebit_asr.infer import seq_logprob

    R, d, V = SCORE_CASES[i]
    h, W, bias, tgt, ref, mx, e_torch = _score_case(i)
    args = [torch.from_numpy(np.ascontiguousarray(a)).to(gpu) for a in (h, W, bias, tgt)]
    lp = seq_logprob(*args)
    assert lp.shape == (R,) and lp.dtype == torch.float32 and lp.is_cuda
    got = lp.cpu().numpy()
    if R == 0:
        return
    err = float(np.abs(got.astype(np.float64) - ref).max())
    bar = max(1e-5 * mx, 4 * e_torch)
    print(f"R={R} d={d} V={V}: max|logit| {mx:.2f} err {err:.3e} e_torch {e_torch:.3e} bar {bar:.3e}")
    assert np.isfinite(got).all()
    assert (got[tgt < 0] == 0.0).all()
    if V == 1:
        assert (got == 0.0).all()
    assert err <= bar
    # bitwise reproducible
    again = seq_logprob(*args).cpu().numpy()
    assert got.tobytes() == again.tobytes()


def test_scorer_reads_no_row_outside_hidden(gpu):
    """hidden [R][d] inside a NaN-filled buffer, NaN guard rows before and after: a read past
    the tile (a row >= R of the last 16-row subtile, a column >= d) would poison a result."""
    from onebit_asr.infer import seq_logprob

    R, d, V = SCORE_CASES[4][0], 144, 5004  # R = 65: a last subtile of one row
    rng = np.random.default_rng(4100)
    h = rng.standard_normal((R, d)).astype(np.float32)
    W = rng.standard_normal((V, d)).astype(np.float32)
    tgt = rng.integers(0, V, size=R).astype(np.int32)
    guard = 32
    buf = torch.full((R + 2 * guard, d), float("nan"), device=gpu)
    buf[guard:guard + R] = torch.from_numpy(h).to(gpu)
    view = buf[guard:guard + R]
    assert view.is_contiguous() and view.data_ptr() % 16 == 0
    Wd = torch.full((V + 2, d), float("nan"), device=gpu)  # the same for the weight's ends
    Wd[1:V + 1] = torch.from_numpy(W).to(gpu)
    got = seq_logprob(view, Wd[1:V + 1], None, torch.from_numpy(tgt).to(gpu)).cpu().numpy()
    ref, mx = rr.seq_logprob(h, W, None, tgt.tolist())
    assert np.isfinite(got).all()
    assert np.abs(got - ref).max() <= 1e-5 * mx


def test_prepare_and_select_kernels_match_the_oracle(gpu):
    """The two small kernels on a hand-sized input, against rescore_ref.prepare / select
    (whose rules test_rescore_cpu.py pins by hand)."""
    from onebit_asr import _lib

    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    B, N, T = 3, 4, 6
    hyps = [[[], [7, 9], [4]], [[5], [4, 6, 8], [9, 9, 9], [5, 6]], [[11, 12, 13, 14, 15, 16]]]
    ctc = np.full((B, N), -np.inf)
    hyp = np.full((B, N, T), -1, np.int32)
    hyp_len = np.zeros((B, N), np.int32)
    n_hyp = np.array([len(u) for u in hyps], np.int32)
    rng = np.random.default_rng(9)
    for b, u in enumerate(hyps):
        for k, y in enumerate(u):
            hyp[b, k, :len(y)] = y
            hyp_len[b, k] = len(y)
            ctc[b, k] = -1.0 - k - rng.random()
    for Lc in (2, 3, 6):
        L1 = Lc + 1
        d_hyp, d_len, d_n = (torch.from_numpy(a).to(gpu) for a in (hyp, hyp_len, n_hyp))
        tgt_inp = torch.full((B * N, L1), -7, dtype=torch.int64, device=gpu)
        target = torch.full((B * N, L1), -7, dtype=torch.int32, device=gpu)
        tgt_pad = torch.full((B * N, L1), 9, dtype=torch.uint8, device=gpu)
        ok = torch.full((B,), 9, dtype=torch.uint8, device=gpu)
        assert lib.ob_rescore_prepare(d_hyp.data_ptr(), d_len.data_ptr(), d_n.data_ptr(), B, N, T,
                                      Lc, 1, 2, 0, tgt_inp.data_ptr(), target.data_ptr(),
                                      tgt_pad.data_ptr(), ok.data_ptr(), st) == 0
        r_inp, r_tgt, r_pad, r_ok = rr.prepare(hyps, N, Lc)
        assert tgt_inp.cpu().tolist() == r_inp and target.cpu().tolist() == r_tgt
        assert tgt_pad.cpu().tolist() == r_pad and ok.cpu().tolist() == r_ok
        lp = -rng.random((B * N, L1)).astype(np.float32)
        lp[1, :] = lp[0, 0] / 2  # utterance 0: entry 1 = 3 equal terms, compared with entry 0
        for w in (0.0, 1.0, 0.5, 1e6):
            out = torch.full((B, T), 5, dtype=torch.int32, device=gpu)
            cnt, best = (torch.full((B,), 77, dtype=torch.int32, device=gpu) for _ in range(2))
            att, tot = (torch.full((B, N), 3.0, dtype=torch.float64, device=gpu) for _ in range(2))
            resc = torch.full((B,), 9, dtype=torch.uint8, device=gpu)
            d_lp, d_ctc = torch.from_numpy(lp).to(gpu), torch.from_numpy(ctc).to(gpu)
            assert lib.ob_rescore_select(d_lp.data_ptr(), d_hyp.data_ptr(), d_len.data_ptr(),
                                         d_n.data_ptr(), d_ctc.data_ptr(), ok.data_ptr(), B, N, T,
                                         Lc, w, out.data_ptr(), cnt.data_ptr(), best.data_ptr(),
                                         att.data_ptr(), tot.data_ptr(), resc.data_ptr(), st) == 0
            ref = rr.select(lp.tolist(), hyps, ctc.tolist(), r_ok, N, w)
            for b, (k, toks, r_att, r_tot, r_resc) in enumerate(ref):
                assert best[b].item() == k and cnt[b].item() == len(toks), (Lc, w, b)
                assert out[b].cpu().tolist() == toks + [-1] * (T - len(toks))
                assert att[b].cpu().tolist() == r_att and tot[b].cpu().tolist() == r_tot
                assert bool(resc[b].item()) == r_resc
    # an exact tie goes to the smaller k (N = 2, both att = -1 - 1, ctc equal)
    hyp2 = torch.tensor([[[4, -1], [5, -1]]], dtype=torch.int32, device=gpu)
    len2 = torch.tensor([[1, 1]], dtype=torch.int32, device=gpu)
    n2 = torch.tensor([2], dtype=torch.int32, device=gpu)
    lp2 = torch.full((2, 2), -1.0, device=gpu)
    ctc2 = torch.tensor([[-3.0, -3.0]], dtype=torch.float64, device=gpu)
    ok2 = torch.ones(1, dtype=torch.uint8, device=gpu)
    out = torch.zeros((1, 2), dtype=torch.int32, device=gpu)
    cnt, best = (torch.zeros(1, dtype=torch.int32, device=gpu) for _ in range(2))
    att, tot = (torch.zeros((1, 2), dtype=torch.float64, device=gpu) for _ in range(2))
    resc = torch.zeros(1, dtype=torch.uint8, device=gpu)
    assert lib.ob_rescore_select(lp2.data_ptr(), hyp2.data_ptr(), len2.data_ptr(), n2.data_ptr(),
                                 ctc2.data_ptr(), ok2.data_ptr(), 1, 2, 2, 1, 0.5, out.data_ptr(),
                                 cnt.data_ptr(), best.data_ptr(), att.data_ptr(), tot.data_ptr(),
                                 resc.data_ptr(), st) == 0
    assert best.item() == 0 and out.cpu().tolist() == [[4, -1]] and tot.cpu().tolist() == [[-3.5, -3.5]]


# ------------------------------------------------------------------------------------------
# end to end
# ------------------------------------------------------------------------------------------
FEAT_LENS, TOK_LENS = [734, 349, 61], [27, 12, 3]


@functools.lru_cache(maxsize=None)
def _model():
    from onebit_asr.conformer import ConformerASR
    from onebit_asr.data import CFG1

    torch.manual_seed(0)
    model = ConformerASR(80, 5004, **CFG1).to("cuda:0").eval()
    return model, rr.double_model(model)


def _lists(info):
    hyp, hyp_len, n_hyp = (info[k].cpu().numpy() for k in ("hyp", "hyp_len", "n_hyp"))
    return [[hyp[b, k, :hyp_len[b, k]].tolist() for k in range(n_hyp[b])]
            for b in range(hyp.shape[0])]


def _existing_path_att(model, info, hyps):
    """The comparator: ``model.decode_logits`` on the GPU (fp32, existing code), log_softmax +
    gather in float64 on the host, each utterance at its own longest hypothesis."""
    enc, mask = info["enc"], info["mask"]
    out = []
    for b, utt in enumerate(hyps):
        n = len(utt)
        inp, tgt, padm, _ = rr.prepare([utt], n, max(len(y) for y in utt))
        z = model.decode_logits(enc[b:b + 1].repeat(n, 1, 1), mask[b:b + 1].repeat(n, 1),
                                torch.tensor(inp, dtype=torch.long, device=enc.device),
                                torch.tensor(padm, dtype=torch.bool, device=enc.device))
        lsm = torch.log_softmax(z.double().cpu(), dim=-1)
        out.append([sum(float(lsm[k, j, tgt[k][j]]) for j in range(len(utt[k]) + 1))
                    for k in range(n)])
    return out


def _check_against_oracle(model, model64, info, out, cnt, w, tag):
    """The end-to-end rule of the module docstring on one run's own encoder output and n-best.
    Returns per utterance (decisive, rescored)."""
    hyps = _lists(info)
    enc, mask = info["enc"].cpu().numpy(), info["mask"].cpu().numpy()
    ctc = info["ctc_scores"].cpu().numpy()
    att_d, tot_d = info["att"].cpu().numpy(), info["total"].cpu().numpy()
    best_d, resc = info["best_k"].cpu().numpy(), info["rescored"].cpu().numpy()
    out, cnt = out.cpu().numpy(), cnt.cpu().numpy()
    att_ref = rr.decoder_scores(model64, enc, mask, hyps)
    with torch.no_grad():
        att_old = _existing_path_att(model, info, hyps)
    e_old = max(abs(a - r) for ao, ar in zip(att_old, att_ref) for a, r in zip(ao, ar))
    inside, flags, e_new = 0, [], 0.0
    for b, utt in enumerate(hyps):
        got = out[b, :cnt[b]].tolist()
        assert (out[b, cnt[b]:] == -1).all()
        if not resc[b]:
            assert best_d[b] == 0 and got == utt[0]
            flags.append((True, False))
            continue
        n = len(utt)
        err = max(abs(att_d[b, k] - att_ref[b][k]) for k in range(n))
        e_new = max(e_new, err)
        tot_ref = [att_ref[b][k] + w * ctc[b, k] for k in range(n)]
        e_tot = max(abs(tot_d[b, k] - tot_ref[k]) for k in range(n))
        order = sorted(range(n), key=lambda k: -tot_ref[k])  # stable: ties to the smaller k
        gap = tot_ref[order[0]] - tot_ref[order[1]] if n > 1 else np.inf
        decisive = gap >= 10 * e_tot
        print(f"{tag} utt {b}: n {n} att err {err:.3e} total err {e_tot:.3e} oracle gap {gap:.3e}"
              f" best_k {best_d[b]} oracle {order[0]}")
        if decisive:
            assert best_d[b] == order[0] and got == utt[order[0]], (b, best_d[b], order[:2])
        else:
            inside += 1
            assert best_d[b] in order[:2] and got == utt[best_d[b]]
        assert (att_d[b, n:] == 0).all() and (tot_d[b, n:] == -np.inf).all()
        flags.append((decisive, True))
    print(f"{tag}: att err new path {e_new:.3e}, existing path {e_old:.3e}, bar {4 * e_old:.3e}")
    assert inside <= 1
    assert e_new <= 4 * e_old
    return flags


def test_rescore_end_to_end_matches_oracle(gpu):
    from onebit_asr.data import synthetic_batch
    from onebit_asr.infer import encode_and_decode

    model, model64 = _model()
    batch = synthetic_batch(FEAT_LENS, TOK_LENS, device=gpu)
    info = {}
    out, cnt, logits = encode_and_decode(model, batch, decoder="rescore", beam_size=10, info=info)
    assert out.dtype == cnt.dtype == torch.int32 and out.shape == logits.shape[:2]
    assert info["hyp"].shape[1] == 10 and info["rescored"].all()
    _check_against_oracle(model, model64, info, out, cnt, 0.5, "eager")
    # an overwhelming CTC weight returns entry 0, which is decoder="beam"
    b_out, b_cnt, _ = encode_and_decode(model, batch, decoder="beam", beam_size=10)
    w_out, w_cnt, _ = encode_and_decode(model, batch, decoder="rescore", beam_size=10,
                                        ctc_weight=1e6)
    assert torch.equal(w_out, b_out) and torch.equal(w_cnt, b_cnt)
    assert torch.equal(info["hyp"][:, 0], b_out) and torch.equal(info["hyp_len"][:, 0], b_cnt)
    # max_len = 5: an utterance with a live hypothesis longer than 5 tokens falls back to its
    # CTC best. The untrained model emits a token on almost every encoder frame (the longest
    # hypotheses here are 182 / 87 / 15 tokens), so at 5 the short utterance falls back as well;
    # max_len = 16 is the mixed case: the two long utterances fall back and the short one is
    # still rescored, to the same winner as at the full length.
    lens = info["hyp_len"].cpu().numpy()
    n_hyp = info["n_hyp"].cpu().numpy()
    longest = [int(lens[b, :n_hyp[b]].max()) for b in range(len(FEAT_LENS))]
    print("longest hypothesis per utterance", longest)
    assert longest[0] > 16 and longest[1] > 16 and 5 < longest[2] <= 16
    for max_len, fits in ((5, [False, False, False]), (16, [False, False, True])):
        info5 = {}
        s_out, s_cnt, _ = encode_and_decode(model, batch, decoder="rescore", beam_size=10,
                                            max_len=max_len, info=info5)
        assert info5["rescored"].cpu().tolist() == fits
        for b, f in enumerate(fits):
            if f:
                assert torch.equal(s_out[b], out[b]) and s_cnt[b] == cnt[b]
                assert info5["best_k"][b] == info["best_k"][b]
                assert abs(float(info5["att"][b, 0] - info["att"][b, 0])) <= 1e-4
            else:
                assert torch.equal(s_out[b], b_out[b]) and s_cnt[b] == b_cnt[b]
                assert info5["best_k"][b] == 0
                assert (info5["att"][b] == 0).all() and (info5["total"][b] == -np.inf).all()


def test_rescore_batch_lists(gpu):
    from onebit_asr.data import synthetic_batch
    from onebit_asr.infer import encode_and_decode
    from onebit_asr.metrics import ctc_attention_rescore_batch

    model, _ = _model()
    batch = synthetic_batch(FEAT_LENS, TOK_LENS, device=gpu)
    out, cnt, _ = encode_and_decode(model, batch, decoder="rescore")
    with torch.no_grad():
        enc, mask, logits = model(batch, precision=2)
    got = ctc_attention_rescore_batch(model, enc, mask, logits, mask.sum(dim=1))
    assert got == [out[b, :cnt[b]].tolist() for b in range(len(FEAT_LENS))]


def test_hidden_fallback_matches_the_grouped_path(gpu):
    """``TransformerDecoder.hidden``: the HIP path with shared memory against its own torch
    fall-back (forced through the parity hook) on repeated memory, and against ``forward``."""
    import onebit_asr.decattn as da

    model, _ = _model()
    dec = model.decoder
    g = torch.Generator().manual_seed(11)
    mem = torch.randn(2, 30, 64, generator=g).to(gpu)
    mmask = torch.ones(2, 30, dtype=torch.long)
    mmask[1, 20:] = 0
    mmask = mmask.to(gpu)
    inp = torch.randint(4, 5004, (6, 7), generator=g)
    inp[:, 0] = 1
    pad = torch.zeros(6, 7, dtype=torch.bool)
    pad[2, 4:] = True
    inp[2, 4:] = 0
    inp, pad = inp.to(gpu), pad.to(gpu)
    h = dec.hidden(inp, mem, mmask, pad, mem_group=3)
    with torch.no_grad():
        z = dec(inp, mem.repeat_interleave(3, 0), mmask.repeat_interleave(3, 0), pad)
        z_h = torch.nn.functional.linear(h, dec.out.weight, dec.out.bias)
    assert (z - z_h).abs().max().item() <= 1e-5 * z.abs().max().item()
    da._ON = False
    try:
        h_t = dec.hidden(inp, mem, mmask, pad, mem_group=3)
    finally:
        da._ON = True
    assert (h - h_t).abs().max().item() <= 1e-5 * h_t.abs().max().item()


def test_graphed_rescore_matches_oracle_and_replays_bitwise(gpu):
    from onebit_asr.data import synthetic_batch
    from onebit_asr.infer import GraphedInference, encode_and_decode
    from onebit_asr.quant import set_act_quant

    model, model64 = _model()
    b1 = synthetic_batch(FEAT_LENS, TOK_LENS, seed=0, device=gpu)
    b2 = synthetic_batch(FEAT_LENS, TOK_LENS, seed=1, device=gpu)
    gi = GraphedInference(model, precision=2, act_quant=None, decoder="rescore", max_len=64)
    runs = []
    for b in (b1, b2, b1):
        out, cnt, logits = gi.run(b)
        runs.append((out.clone(), cnt.clone(), logits.clone(),
                     {k: v.clone() for k, v in gi.info.items()}))
    assert gi.graph is not None
    set_act_quant(model, None)
    for tag, b, (out, cnt, logits, info) in zip(("g1", "g2", "g3"), (b1, b2, b1), runs):
        e_info = {}
        e_out, e_cnt, e_logits = encode_and_decode(model, b, precision=2, decoder="rescore",
                                                   max_len=64, info=e_info)
        # MIOpen may pick other conv solvers under capture: rounding-level differences
        assert (logits - e_logits).abs().max().item() <= 1e-4 * e_logits.abs().max().item()
        if tag == "g3":
            continue  # (bitwise run 1, below)
        g_flags = _check_against_oracle(model, model64, info, out, cnt, 0.5, tag)
        e_flags = _check_against_oracle(model, model64, e_info, e_out, e_cnt, 0.5, tag + "-eager")
        same = torch.equal(info["hyp"], e_info["hyp"])
        for u, ((gd, gr), (ed, er)) in enumerate(zip(g_flags, e_flags)):
            if same and gd and ed:
                assert gr == er and torch.equal(out[u], e_out[u]) and cnt[u] == e_cnt[u]
    # the first and the third run saw the same batch: the same bits
    for a, c in zip(runs[0][:3], runs[2][:3]):
        assert torch.equal(a, c)
    for k in ("best_k", "att", "total", "rescored", "hyp", "ctc_scores"):
        assert runs[0][3][k].cpu().numpy().tobytes() == runs[2][3][k].cpu().numpy().tobytes(), k


@pytest.mark.parametrize("decoder", ["greedy", "beam"])
def test_graphed_greedy_and_beam_are_unchanged(gpu, decoder):
    from onebit_asr.data import synthetic_batch
    from onebit_asr.infer import (GraphedInference, ctc_beam_search_batch_device,
                                  ctc_greedy_decode_batch, encode_and_decode)
    from onebit_asr.quant import set_act_quant

    model, _ = _model()
    b1 = synthetic_batch(FEAT_LENS, TOK_LENS, seed=0, device=gpu)
    gi = GraphedInference(model, precision=2, act_quant=None, decoder=decoder)
    out, cnt, logits = (t.clone() for t in gi.run(b1))
    set_act_quant(model, None)
    e_out, e_cnt, e_logits = encode_and_decode(model, b1, precision=2, decoder=decoder)
    assert (logits - e_logits).abs().max().item() <= 1e-4 * e_logits.abs().max().item()
    with torch.no_grad():
        lens = model(b1, precision=2)[1].sum(dim=1)
    for lg, o, c in ((logits, out, cnt), (e_logits, e_out, e_cnt)):
        if decoder == "beam":
            r_out, r_cnt, _ = ctc_beam_search_batch_device(lg, lens, 10, BLANK)
        else:
            r_out, r_cnt = ctc_greedy_decode_batch(lg, lens, BLANK)
        assert torch.equal(o, r_out) and torch.equal(c, r_cnt)
