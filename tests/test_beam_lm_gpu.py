"""GPU: ob_ctc_beam_search_lm (csrc/beam.hip), the CTC prefix beam search with the n-gram LM inside
it, against the fp64 oracle of tests/ctc_beam_lm_ref.py.

The rule is test_beam_search_gpu.py's: both sides are fp64 from the same fp32 logits, so ``ctc``
agrees to 1e-9 * max(1, T); where the oracle's smallest decision margin (top-k boundary, prune
boundary in the key, final best against the runner-up in the total) is >= 1e-6 the best
hypothesis, its length and the -1 padding are exactly the oracle's. The LM term is a sum of
float32 table values in a fixed order: it is compared bit for bit, with the oracle and with the
host scorer, and ``total`` bit for bit with its formula over the device's own outputs.
"""
import functools

import numpy as np
import pytest
import torch

import ngram_ref as nr
from ctc_beam_lm_ref import lm_beam_search, lm_beam_search_batch
from ctc_beam_ref import beam_search, ctc_like_logits, ragged_lens

pytestmark = pytest.mark.gpu

BLANK = 3
MARGIN = 1e-6

#         B   T    V   beam top_k order lm_weight ins_bonus
CASES = [(1, 1, 5, 10, 20, 2, 0.5, 0.0),
         (3, 17, 7, 10, 20, 3, 0.3, 0.5),
         (4, 64, 40, 10, 20, 4, 0.5, 0.0),
         (2, 16, 5004, 10, 20, 4, 0.3, 1.0),    # the real vocabulary, the 200k-entry table
         (4, 33, 40, 4, 20, 3, 1.0, 0.0),
         (4, 64, 40, 1, 20, 2, 0.5, 0.0),
         (3, 48, 70, 16, 32, 4, 0.2, 0.5),
         (2, 40, 12, 32, 20, 3, 0.5, 0.0)]      # more beam than a frame can fill early on
IDS = ["-".join(map(str, c)) for c in CASES]


def _bits(x):
    return np.asarray(x, np.float64).view(np.int64)


@functools.lru_cache(maxsize=None)
def _tables(i):
    """-> (RefLM, (ids, n, vals)) of CASES[i]."""
    _, _, V, _, _, order, _, _ = CASES[i]
    if V == 5004:
        ref, ids, n, vals = nr.big_lm()
        assert ref.order == order
    else:
        entries, ids, n, vals = nr.random_lm(300 + i, order, V, 40 * V)
        ref = nr.RefLM(entries, order)
    return ref, (ids, n, vals)


@functools.lru_cache(maxsize=None)
def _lm(i):
    from onebit_asr.ngram import NGramLM

    ref, (ids, n, vals) = _tables(i)
    return NGramLM.from_arrays(ids, n, vals, ref.order)


@functools.lru_cache(maxsize=None)
def _case(i):
    """Inputs and the oracle's results of CASES[i]: computed once, shared, never modified."""
    B, T, V, beam, top_k, order, lw, bonus = CASES[i]
    logits = ctc_like_logits(2000 + i, B, T, V, BLANK)
    lens = ragged_lens(2000 + i, B, T)
    logits.setflags(write=False)
    lens.setflags(write=False)
    refs = lm_beam_search_batch(logits, lens, _tables(i)[0], lw, bonus, beam, BLANK, top_k)
    return logits, lens, tuple(refs)


def _device(i, gpu, nbest=None, lw=None, bonus=None):
    from onebit_asr.infer import ctc_beam_search_lm_device

    B, T, V, beam, top_k, _, lw0, bonus0 = CASES[i]
    logits, lens, _ = _case(i)
    hyp, hyp_len, n_hyp, info = ctc_beam_search_lm_device(
        torch.from_numpy(np.ascontiguousarray(logits)).to(gpu), torch.from_numpy(lens).to(gpu),
        _lm(i), lw0 if lw is None else lw, bonus0 if bonus is None else bonus, beam_size=beam,
        nbest=nbest, blank_id=BLANK, top_k_per_t=top_k)
    nb = beam if nbest is None else nbest
    assert hyp.dtype == hyp_len.dtype == n_hyp.dtype == torch.int32
    assert hyp.shape == (B, nb, T) and hyp_len.shape == (B, nb) and n_hyp.shape == (B,)
    assert set(info) == {"ctc", "lm", "total"}
    for v in info.values():
        assert v.dtype == torch.float64 and v.shape == (B, nb) and v.is_cuda
    return (hyp.cpu().numpy(), hyp_len.cpu().numpy(), n_hyp.cpu().numpy(),
            {k: v.cpu().numpy() for k, v in info.items()})


def _tokens(hyp, hyp_len, b, k):
    return hyp[b, k, :hyp_len[b, k]].tolist()


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_fused_search_matches_oracle(gpu, i):
    B, T, V, beam, top_k, order, lw, bonus = CASES[i]
    logits, lens, refs = _case(i)
    assert lens[0] == T and (B == 1 or lens[-1] == 0)
    # the condition on the test itself, from the oracle alone
    assert sum(r.margin < MARGIN for r in refs) <= B // 16
    if i in (1, 2, 4, 6, 7):                     # extensions land on live prefixes there
        assert sum(r.merges for r in refs) > 0
    hyp, hyp_len, n_hyp, info = _device(i, gpu)
    lm = _lm(i)
    low = 0
    for b, r in enumerate(refs):
        n = int(n_hyp[b])
        assert n == len(r.beam), (b, n, len(r.beam))
        for k in range(beam):
            m = int(hyp_len[b, k])
            assert 0 <= m <= T and (hyp[b, k, m:] == -1).all() and (hyp[b, k, :m] >= 0).all()
            if k >= n:
                assert m == 0 and all(info[f][b, k] == -np.inf for f in info), (b, k)
                continue
            # total: its formula over the device's own outputs, each operation rounded
            want = (info["ctc"][b, k] + np.float64(lw) * info["lm"][b, k]) \
                + np.float64(bonus) * np.float64(m)
            assert _bits(info["total"][b, k]) == _bits(want), (b, k)
        assert (np.diff(info["total"][b, :n]) <= 0).all(), b
        toks, ctc, lm_fin, total = r.beam[0]
        got = _tokens(hyp, hyp_len, b, 0)
        err = abs(float(info["ctc"][b, 0]) - ctc)
        print(f"utt {b}: margin {r.margin:.3e} gap {r.gap:.3e} merges {r.merges} ctc err {err:.3e} "
              f"n {len(got)} ref n {len(toks)}")
        if r.margin < MARGIN:
            low += 1
            assert got in r.final_beam, (b, got)
            continue
        assert got == toks, (b, got, toks)
        assert err <= 1e-9 * max(1, T), (b, float(info["ctc"][b, 0]), ctc)
        assert _bits(info["lm"][b, 0]) == _bits(lm_fin), (b, float(info["lm"][b, 0]), lm_fin)
        assert _bits(lm.seq_logprob(got)) == _bits(info["lm"][b, 0]), b
        if lens[b] == 0:
            assert got == [] and n == 1 and info["ctc"][b, 0] == 0.0
            assert _bits(info["lm"][b, 0]) == _bits(lm.score([], lm.eos))
        if r.gap >= MARGIN:     # every adjacent pair of totals is apart: the whole order
            assert [_tokens(hyp, hyp_len, b, k) for k in range(n)] == r.final_beam, b
            for k, (_, c_k, l_k, _) in enumerate(r.beam):
                assert abs(float(info["ctc"][b, k]) - c_k) <= 1e-9 * max(1, T), (b, k)
                assert _bits(info["lm"][b, k]) == _bits(l_k), (b, k)
    assert low <= B // 16


@pytest.mark.parametrize("i", [2, 7], ids=[IDS[2], IDS[7]])
def test_zero_weights_are_the_plain_nbest_bit_for_bit(gpu, i):
    from onebit_asr.infer import ctc_beam_search_nbest_device

    B, T, V, beam, top_k = CASES[i][:5]
    logits, lens, _ = _case(i)
    hyp, hyp_len, n_hyp, info = _device(i, gpu, lw=0.0, bonus=0.0)
    p_hyp, p_len, p_n, p_score = ctc_beam_search_nbest_device(
        torch.from_numpy(np.ascontiguousarray(logits)).to(gpu), torch.from_numpy(lens).to(gpu),
        beam_size=beam, blank_id=BLANK, top_k_per_t=top_k)
    assert (hyp == p_hyp.cpu().numpy()).all() and (hyp_len == p_len.cpu().numpy()).all()
    assert (n_hyp == p_n.cpu().numpy()).all()
    assert (_bits(info["ctc"]) == _bits(p_score.cpu().numpy())).all()


class _FixedLogits:
    """Stands in for the model in encode_and_decode: the batch's own logits and mask."""

    def __call__(self, batch, precision=2):
        return None, batch["mask"], batch["logits"]


@pytest.mark.parametrize("i", [2, 4, 7], ids=[IDS[2], IDS[4], IDS[7]])
def test_fusion_finds_what_reranking_cannot(gpu, i):
    from onebit_asr.infer import encode_and_decode

    B, T, V, beam, top_k, order, lw, bonus = CASES[i]
    assert bonus == 0.0 and top_k == 20          # what encode_and_decode's re-ranking runs with
    logits, lens, refs = _case(i)
    ref_lm = _tables(i)[0]
    live = [b for b in range(B) if lens[b] > 0]
    assert live
    for b in live:                               # the CPU side: re-ranking cannot reach the best
        r = refs[b]
        plain = beam_search(logits[b, :lens[b]], beam, BLANK, top_k)
        assert r.tokens not in plain.final_beam, b
        # the plain search again through the fused oracle (weights 0: the same beam), which also
        # reports every entry's ctc and lm: what re-ranking chooses from
        zero = lm_beam_search(logits[b, :lens[b]], ref_lm, 0.0, 0.0, beam, BLANK, top_k)
        assert zero.final_beam == plain.final_beam
        reach = max(ctc + lw * lm_fin for _, ctc, lm_fin, _ in zero.beam)
        print(f"utt {b}: fused total {r.beam[0][3]:.4f}, best re-ranked {reach:.4f}")
        assert r.beam[0][3] > reach + 1.0, (b, r.beam[0][3], reach)
        assert r.margin >= MARGIN
    hyp, hyp_len, n_hyp, info = _device(i, gpu)
    mask = torch.arange(T)[None, :] < torch.from_numpy(lens)[:, None]
    batch = {"logits": torch.from_numpy(np.ascontiguousarray(logits)).to(gpu),
             "mask": mask.to(gpu).long()}
    out, cnt, _ = encode_and_decode(_FixedLogits(), batch, decoder="beam", beam_size=beam,
                                    blank_id=BLANK, lm=_lm(i), lm_weight=lw, lm_fusion="rescore")
    out, cnt = out.cpu().numpy(), cnt.cpu().numpy()
    for b in live:
        assert _tokens(hyp, hyp_len, b, 0) == refs[b].tokens, b
        assert out[b, :cnt[b]].tolist() != refs[b].tokens, b


def test_a_merge_keeps_one_lm_value(gpu):
    i = 7
    B, T, V, beam = CASES[i][:4]
    logits, lens, refs = _case(i)
    assert sum(r.merges for r in refs) >= 100
    hyp, hyp_len, n_hyp, info = _device(i, gpu, nbest=beam)
    lm = _lm(i)
    for b in range(B):
        n = int(n_hyp[b])
        got = [tuple(_tokens(hyp, hyp_len, b, k)) for k in range(n)]
        assert len(set(got)) == n, b
        for k in range(n):
            assert _bits(info["lm"][b, k]) == _bits(lm.seq_logprob(got[k])), (b, k)


@functools.lru_cache(maxsize=None)
def _model():
    from onebit_asr.conformer import ConformerASR
    from onebit_asr.data import CFG1, synthetic_batch
    from onebit_asr.ngram import NGramLM

    torch.manual_seed(0)
    model = ConformerASR(80, 5004, **CFG1).to("cuda:0").eval()
    batches = [synthetic_batch([734, 349], [27, 12], seed=s, device="cuda:0") for s in (0, 1)]
    ref, ids, n, vals = nr.big_lm()
    return model, batches, NGramLM.from_arrays(ids, n, vals, ref.order)


KEYS = ("hyp", "hyp_len", "n_hyp", "ctc_scores", "lm", "total", "best_k")


def _same(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape
    assert a.contiguous().view(torch.uint8).equal(b.contiguous().view(torch.uint8))


def test_first_pass_in_encode_and_decode_and_graphed(gpu):
    from onebit_asr.infer import (GraphedInference, ctc_beam_search_lm_device, ctc_lm_rescore,
                                  ctc_beam_search_nbest_device, encode_and_decode)
    from onebit_asr.quant import set_act_quant

    model, (b1, b2), lm = _model()
    kw = dict(decoder="beam", beam_size=4, lm=lm, lm_weight=0.4)
    fp = dict(kw, lm_fusion="first_pass", ins_bonus=0.5)
    gi = GraphedInference(model, act_quant=None, timestamps=True, **fp)
    runs = []
    for b in (b1, b2, b1):
        out, cnt, logits = gi.run(b)
        runs.append([out.clone(), cnt.clone(), logits.clone(),
                     {k: gi.info[k].clone() for k in KEYS + ("align_score",)}])
    assert gi.graph is not None
    assert not torch.equal(runs[0][2], runs[1][2])          # the replay saw the second batch
    set_act_quant(model, None)
    for b, run in ((b1, runs[0]), (b2, runs[1]), (b1, runs[2])):
        info = {}
        out, cnt, logits = encode_and_decode(model, b, info=info, timestamps=True, **fp)
        assert set(info) >= set(KEYS) | {"span", "tok_score", "align_score", "frame_path"}
        for x, y in zip((out, cnt, logits), run[:3]):
            _same(x, y)
        for k in run[3]:
            _same(info[k], run[3][k])
        # the result is the plain call on the returned logits, entry 0
        lens = (b["feat_lens"] // 4).clamp(max=logits.size(1))
        hyp, hyp_len, n_hyp, res = ctc_beam_search_lm_device(logits, lens, lm, 0.4, 0.5, 4)
        for x, y in ((info["hyp"], hyp), (info["hyp_len"], hyp_len), (info["n_hyp"], n_hyp),
                     (info["ctc_scores"], res["ctc"]), (info["lm"], res["lm"]),
                     (info["total"], res["total"]), (out, hyp[:, 0].contiguous()),
                     (cnt, hyp_len[:, 0].contiguous())):
            _same(x, y)
        assert (info["best_k"] == 0).all()
        assert torch.isfinite(info["align_score"][cnt > 0]).all()
        # the default is today's re-ranking of the plain n-best, bit for bit
        d_info, r_info = {}, {}
        d = encode_and_decode(model, b, info=d_info, **kw)
        r = encode_and_decode(model, b, info=r_info, lm_fusion="rescore", **kw)
        n_h, n_l, n_n, n_s = ctc_beam_search_nbest_device(d[2], lens, 4)
        t_out, t_cnt, t_res = ctc_lm_rescore(n_h, n_l, n_n, n_s, lm, 0.4, 5004)
        for x, y, z in zip(d[:2], r[:2], (t_out, t_cnt)):
            _same(x, y)
            _same(x, z)
        assert d_info.keys() == r_info.keys()
        for k in ("best_k", "lm", "total"):
            _same(d_info[k], t_res[k])
            _same(d_info[k], r_info[k])
