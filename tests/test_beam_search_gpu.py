"""GPU: ob_ctc_beam_search (csrc/beam.hip) against the fp64 oracle of tests/ctc_beam_ref.py.

Both sides are fp64 from the same fp32 logits, so scores must agree to 1e-9 * max(1, T) (over
100x the rounding of about 20 double operations per frame plus a V-term sum). Where the
oracle's smallest decision margin is >= 1e-6 the hypothesis, its count and the -1 padding must
be exactly the oracle's; below that the hypothesis must be one of the oracle's final beam. The
seeds are chosen so that the oracle alone shows at most 1 low-margin utterance in 16 per case
(asserted below, on the CPU side of each test).
"""
import functools
import json

import numpy as np
import pytest
import torch

from ctc_beam_ref import (beam_search, beam_search_batch, beam_search_fresh_ids, ctc_like_logits,
                          ragged_lens)

pytestmark = pytest.mark.gpu

BLANK = 3
MARGIN = 1e-6

#         B   T    V   beam top_k
CASES = [(1, 1, 5, 10, 20),
         (3, 17, 7, 10, 20),      # all-token candidates, blank inside
         (4, 64, 40, 10, 20),
         (2, 16, 5004, 10, 20),   # the real vocabulary
         (4, 33, 40, 4, 20),
         (4, 64, 40, 1, 20),
         (3, 48, 70, 16, 32),
         (2, 40, 12, 32, 20)]     # more beam than a frame can fill early on


@functools.lru_cache(maxsize=None)
def _case(i):
    """Inputs and the oracle's results of CASES[i]: computed once, shared, never modified."""
    B, T, V, beam, top_k = CASES[i]
    logits = ctc_like_logits(1000 + i, B, T, V, BLANK)
    lens = ragged_lens(1000 + i, B, T)
    logits.setflags(write=False)
    lens.setflags(write=False)
    return logits, lens, tuple(beam_search_batch(logits, lens, beam, BLANK, top_k))


def _device(logits, lens, gpu, beam, top_k, blank=BLANK):
    from onebit_asr.infer import ctc_beam_search_batch_device

    out, cnt, score = ctc_beam_search_batch_device(
        torch.from_numpy(np.ascontiguousarray(logits)).to(gpu), torch.from_numpy(np.asarray(lens)).to(gpu),
        beam_size=beam, blank_id=blank, top_k_per_t=top_k)
    assert out.dtype == torch.int32 and cnt.dtype == torch.int32 and score.dtype == torch.float64
    assert out.is_cuda and cnt.is_cuda and score.is_cuda
    assert out.shape == logits.shape[:2] and cnt.shape == score.shape == logits.shape[:1]
    return out.cpu().numpy(), cnt.cpu().numpy(), score.cpu().numpy()


def _check(out, cnt, score, refs, T):
    """The per-utterance rule of the module docstring; returns the number of low-margin ones."""
    low = 0
    for b, r in enumerate(refs):
        n = int(cnt[b])
        err = abs(float(score[b]) - r.score)
        print(f"utt {b}: margin {r.margin:.3e} score err {err:.3e} n {n} ref n {len(r.tokens)}")
        assert err <= 1e-9 * max(1, T), (b, float(score[b]), r.score)
        assert 0 <= n <= T
        assert (out[b, n:] == -1).all(), b
        hyp = out[b, :n].tolist()
        if r.margin >= MARGIN:
            assert hyp == r.tokens, (b, hyp, r.tokens)
        else:
            low += 1
            assert hyp in r.final_beam, (b, hyp, r.final_beam)
    return low


@pytest.mark.parametrize("i", range(len(CASES)), ids=["-".join(map(str, c)) for c in CASES])
def test_beam_search_matches_oracle(gpu, i):
    B, T, V, beam, top_k = CASES[i]
    logits, lens, refs = _case(i)
    assert lens[0] == T and (B == 1 or lens[-1] == 0)
    # the condition on the test itself, from the oracle alone
    assert sum(r.margin < MARGIN for r in refs) <= B // 16
    out, cnt, score = _device(logits, lens, gpu, beam, top_k)
    assert _check(out, cnt, score, refs, T) <= B // 16
    for b in range(B):
        if lens[b] == 0:
            assert cnt[b] == 0 and score[b] == 0.0


def test_prefix_identity_when_a_pruned_prefix_returns(gpu):
    """A pruned prefix is built again from its parent while a child of its first copy is still
    live, and is then extended onto that child: both copies must be one prefix (canonical ids),
    or the merge is missed and the mass is split. ``beam_search_fresh_ids`` is the search with
    that mistake; the input is pinned where it gives another hypothesis than the oracle."""
    B, T, V, beam, top_k = 4, 48, 12, 4, 20
    logits = ctc_like_logits(3050, B, T, V, BLANK)
    lens = np.full(B, T, np.int64)
    refs = beam_search_batch(logits, lens, beam, BLANK, top_k)
    # the CPU side: the case is there, and a fresh-id search fails it by far more than the
    # tolerance below (so it cannot silently disappear)
    assert [r.reentries for r in refs] == [0, 1, 0, 0]
    assert all(r.margin >= 1e-4 for r in refs)
    wrong = [beam_search_fresh_ids(logits[b], beam, BLANK, top_k) for b in range(B)]
    assert [w.merges for w in wrong] == [0, 1, 0, 0]  # merges that fresh ids miss
    assert wrong[1].tokens != refs[1].tokens
    assert abs(wrong[1].score - refs[1].score) > 0.1  # the bound on the device is 4.8e-8
    out, cnt, score = _device(logits, lens, gpu, beam, top_k)
    assert _check(out, cnt, score, refs, T) == 0


def test_top_k_tie_at_the_boundary(gpu):
    """Bit-equal logits at ranks K and K + 1: the lower token index is a candidate."""
    T, V, K, beam = 6, 12, 2, 10
    rng = np.random.default_rng(5)
    logits = rng.standard_normal((2, T, V)).astype(np.float32)
    logits[0, :, BLANK] -= 4.0  # few blanks: every frame shows in the result
    logits[0, :, [6, 9]] = -9.0
    # utterance 0: frame 1 is token 0; in frame 2 token 0 is rank 1 again (a repeat, which does
    # not extend the prefix) and tokens 6 and 9 tie bit for bit for rank 2 = K, so which of them
    # is a candidate decides the hypothesis
    logits[0, 1:3] = -8.0
    logits[0, 1, 0] = 4.0
    logits[0, 2, 0] = 4.0
    logits[0, 2, [9, 6]] = 3.0
    lens = np.array([T, T], np.int64)
    refs = beam_search_batch(logits, lens, beam, BLANK, K)
    assert refs[0].margin == 0.0  # the tie is on the boundary
    assert refs[0].tokens[:3] == [4, 0, 6]  # 6 entered, 9 did not
    assert not any(9 in p for p in refs[0].final_beam)
    out, cnt, score = _device(logits, lens, gpu, beam, K)
    for b in range(2):
        assert out[b, :cnt[b]].tolist() == refs[b].tokens
        assert abs(score[b] - refs[b].score) <= 1e-9 * T
    # token 6 lowered: the pair no longer ties and token 9 holds rank 2 on its own
    swapped = logits.copy()
    swapped[0, 2, 6] = 2.0
    r = beam_search(swapped[0], beam, BLANK, K)
    out, cnt, _ = _device(swapped, lens, gpu, beam, K)
    assert out[0, :cnt[0]].tolist() == r.tokens and r.tokens[:3] == [4, 0, 9]


def test_goldens_on_the_device(gpu, golden_dir):
    kat = json.loads((golden_dir / "beam_kat.json").read_text())
    x = np.stack([np.asarray(c["logits"], np.float32) for c in kat["cases"] if len(c["logits"]) == 3])
    three = [c for c in kat["cases"] if len(c["logits"]) == 3]
    lens = np.array([c["len"] for c in three], np.int64)
    out, cnt, score = _device(x, lens, gpu, kat["beam_size"], kat["top_k_per_t"], kat["blank_id"])
    for b, c in enumerate(three):
        assert out[b, :cnt[b]].tolist() == c["tokens"], c["name"]
        if c["score"] is not None:
            assert abs(score[b] - c["score"]) <= 1e-9 * 3, c["name"]
    for c in kat["cases"]:
        if len(c["logits"]) == 3:
            continue
        x = np.asarray(c["logits"], np.float32)[None]
        out, cnt, score = _device(x, np.array([c["len"]]), gpu, kat["beam_size"], kat["top_k_per_t"],
                                  kat["blank_id"])
        assert out[0, :cnt[0]].tolist() == c["tokens"], c["name"]
        assert c["score"] is None or abs(score[0] - c["score"]) <= 1e-9 * x.shape[1]

    ref = json.loads((golden_dir / "beam_ref.json").read_text())
    T = max(c["T"] for c in ref["cases"])
    x = np.zeros((len(ref["cases"]), T, 24), np.float32)
    for b, c in enumerate(ref["cases"]):
        x[b, :c["T"]] = np.asarray(c["logits"], np.float32)
    lens = np.array([c["T"] for c in ref["cases"]], np.int64)
    out, cnt, _ = _device(x, lens, gpu, 10, 20)
    for b, c in enumerate(ref["cases"]):
        assert out[b, :cnt[b]].tolist() == c["tokens"], c["seed"]  # the reference's own output


def test_determinism(gpu):
    from onebit_asr.infer import ctc_beam_search_batch_device

    logits, lens, _ = _case(2)
    x, ln = torch.from_numpy(logits).to(gpu), torch.from_numpy(lens).to(gpu)
    a = ctc_beam_search_batch_device(x, ln)
    b = ctc_beam_search_batch_device(x, ln)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    assert a[2].view(torch.int64).equal(b[2].view(torch.int64))  # scores: the same bits


def test_stages_on_their_own(gpu):
    """ob_ctc_beam_search_stage: frames (1) then search (2) equals the single call, and the
    search alone decodes the same candidates again at another beam size."""
    from onebit_asr import _lib
    from onebit_asr.infer import ctc_beam_search_batch_device

    lib = _lib.load()
    B, T, V, beam, top_k = CASES[2]
    logits, lens, refs = _case(2)
    x, ln = torch.from_numpy(logits).to(gpu), torch.from_numpy(lens).to(gpu)
    need = lib.ob_ctc_beam_search_workspace(B, T, V, beam, top_k)
    ws = torch.empty(need // 8, dtype=torch.int64, device=gpu)
    out = torch.full((B, T), -7, dtype=torch.int32, device=gpu)
    cnt = torch.full((B,), -7, dtype=torch.int32, device=gpu)
    score = torch.zeros(B, dtype=torch.float64, device=gpu)

    def stage(k, beam_k, logits_ptr, outs):
        _lib.check(lib.ob_ctc_beam_search_stage(logits_ptr, ln.data_ptr(), B, T, V, BLANK, beam_k,
                                                top_k, k, ws.data_ptr(), need, *outs,
                                                _lib.stream_of(x)), "stage")

    stage(1, beam, x.data_ptr(), (None, None, None))
    assert (out == -7).all() and (cnt == -7).all()  # stage 1 leaves the outputs alone
    stage(2, beam, None, (out.data_ptr(), cnt.data_ptr(), score.data_ptr()))
    for u, v in zip((out, cnt, score), ctc_beam_search_batch_device(x, ln, beam, BLANK, top_k)):
        assert torch.equal(u, v)
    stage(2, 4, None, (out.data_ptr(), cnt.data_ptr(), score.data_ptr()))  # a smaller table fits
    r4 = beam_search_batch(logits, lens, 4, BLANK, top_k)
    assert all(r.margin >= MARGIN for r in r4)
    assert _check(out.cpu().numpy(), cnt.cpu().numpy(), score.cpu().numpy(), r4, T) == 0


@pytest.mark.parametrize("top_k", [None, 3])
def test_one_best_without_score_and_nbest_one(gpu, top_k):
    """The three forms share one launcher and one checked entry, the 1-best with no n_hyp and an
    optional score: a null score changes nothing else, nbest == 1 is the 1-best call bytewise, and
    the result is the oracle's -- with an empty utterance, a one-frame one, and a -1 fill longer
    than a wave."""
    from onebit_asr import _lib
    from onebit_asr.infer import ctc_beam_search_batch_device, ctc_beam_search_nbest_device

    B, T, V, beam = 3, 70, 6, 4
    logits = ctc_like_logits(4100, B, T, V, BLANK)
    lens = np.array([T, 0, 1], np.int64)
    refs = beam_search_batch(logits, lens, beam, BLANK, top_k)
    x, ln = torch.from_numpy(logits).to(gpu), torch.from_numpy(lens).to(gpu)
    out, cnt, score = ctc_beam_search_batch_device(x, ln, beam, BLANK, top_k)

    # (a) the raw entry without a score buffer
    lib = _lib.load()
    K = V if top_k is None else top_k
    need = lib.ob_ctc_beam_search_workspace(B, T, V, beam, K)
    ws = torch.empty(need // 8, dtype=torch.int64, device=gpu)
    out0 = torch.full((B, T), -7, dtype=torch.int32, device=gpu)
    cnt0 = torch.full((B,), -7, dtype=torch.int32, device=gpu)
    assert lib.ob_ctc_beam_search(x.data_ptr(), ln.data_ptr(), B, T, V, BLANK, beam, K,
                                  ws.data_ptr(), need, out0.data_ptr(), cnt0.data_ptr(), None,
                                  _lib.stream_of(x)) == 0
    assert torch.equal(out0, out) and torch.equal(cnt0, cnt)

    # (b) the n-best at nbest == 1
    hyp, hyp_len, n_hyp, nscore = ctc_beam_search_nbest_device(x, ln, beam, 1, BLANK, top_k)
    assert hyp.shape == (B, 1, T) and hyp_len.shape == nscore.shape == (B, 1)
    assert torch.equal(hyp[:, 0], out) and torch.equal(hyp_len[:, 0], cnt)
    assert nscore[:, 0].contiguous().view(torch.int64).equal(score.view(torch.int64))
    assert n_hyp.tolist() == [min(1, len(r.final_beam)) for r in refs] == [1, 1, 1]

    # (c) the oracle, exactly: no decision of it is close on these inputs
    assert all(r.margin >= MARGIN for r in refs) and len(refs[0].tokens) > 1
    assert _check(out.cpu().numpy(), cnt.cpu().numpy(), score.cpu().numpy(), refs, T) == 0
    assert cnt[1] == 0 and score[1] == 0.0 and (out[1:, 1:] == -1).all()


def test_metrics_signatures(gpu):
    from onebit_asr import metrics

    logits, lens, refs = _case(2)
    x = torch.from_numpy(logits).to(gpu)
    got = metrics.ctc_beam_search_batch(x, torch.from_numpy(lens).to(gpu))
    assert isinstance(got, list) and all(isinstance(g, list) for g in got)
    assert got == [r.tokens for r in refs]
    one = metrics.ctc_beam_search(x[0])
    assert isinstance(one, list) and all(isinstance(t, int) for t in one) and one == refs[0].tokens
    assert metrics.ctc_beam_search(x[0], beam_size=4, top_k_per_t=8) == \
        beam_search(logits[0], 4, BLANK, 8).tokens
    l12, n12, _ = _case(7)  # V = 12: no top-k limit is allowed
    r = beam_search(l12[0], 10, BLANK, None)
    assert r.margin >= MARGIN
    assert metrics.ctc_beam_search(torch.from_numpy(l12[0]).to(gpu), top_k_per_t=None) == r.tokens
    l70, _, _ = _case(6)  # V = 70: more than the 64 candidates a frame can hold
    with pytest.raises(ValueError, match="V <= 64"):
        metrics.ctc_beam_search(torch.from_numpy(l70[0]).to(gpu), top_k_per_t=None)
    with pytest.raises(ValueError):
        metrics.ctc_beam_search(x[0], beam_size=33)
    assert metrics.ctc_greedy_decode(x[0]) == metrics.ctc_greedy_decode(x[0].clone())


def test_graphed_beam_inference_matches_eager(gpu):
    from onebit_asr.conformer import ConformerASR
    from onebit_asr.data import CFG1, synthetic_batch
    from onebit_asr.infer import GraphedInference, encode_and_decode

    torch.manual_seed(0)
    model = ConformerASR(80, 5004, **CFG1).to(gpu).eval()
    b1 = synthetic_batch([734, 349], [27, 12], seed=0, device=gpu)
    b2 = synthetic_batch([734, 349], [27, 12], seed=1, device=gpu)
    gi = GraphedInference(model, precision=2, decoder="beam")
    got = [tuple(t.clone() for t in gi.run(b)) for b in (b1, b2)]
    assert not torch.equal(got[0][2], got[1][2])  # the replay saw the second batch
    from onebit_asr.infer import ctc_beam_search_batch_device

    low = 0
    for b, (out, cnt, logits) in zip((b1, b2), got):
        e_out, e_cnt, e_logits = encode_and_decode(model, b, precision=2, decoder="beam")
        T = logits.size(1)
        lens_t = (b["feat_lens"] // 4).clamp(max=T)
        lens = lens_t.cpu().numpy()
        for o, c, lg in ((out, cnt, logits), (e_out, e_cnt, e_logits)):
            # the decode inside the graph / the eager call equals the plain call on its logits,
            # which also gives the scores that encode_and_decode drops
            o2, c2, sc = ctc_beam_search_batch_device(lg, lens_t)
            assert torch.equal(o, o2) and torch.equal(c, c2)
            refs = beam_search_batch(lg.cpu().numpy(), lens, 10, BLANK, 20)
            low += _check(o.cpu().numpy(), c.cpu().numpy(), sc.cpu().numpy(), refs, T)
    assert low <= 1, low  # of 8 decoded utterances: the rest are compared exactly
