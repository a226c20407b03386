"""GPU: the device edit distance (csrc/edit.hip, onebit_asr/edit.py) against tests/edit_ref.py.

1. ``edit_distance``: dist and ops exact, lengths on both sides of every 64-row band boundary,
   tight widths and slack widths with live-looking padding, alphabets of 2 and 5004 symbols,
   identical and absent pairs; one pair at the limit (4096 x 4000 tokens), distance only.
2. ``nbest_edit_distance``: dref / ops / dpair exact; dpair symmetric with a zero live diagonal
   and -1 for absent entries; dref / ops bit for bit the per-pair call's; ``nbest_oracle``.
3. ``mbr_select``: post and risk within rtol 1e-11 (the only inexact step is the fp64 exp, a few
   ulp times an argument of at most a few hundred, then sums of at most 32 terms: about 1e-13); the
   pick is a valid argmin of the oracle's risk for every utterance (within 1e-9), and equal to
   the oracle's k at scale > 0: there the oracle's two smallest risks are at least 4.2e-3 apart
   among the 64 utterances of this generator with two live entries or more, except for 26 exact
   ties, every one between identical entries, whose risks are the same sums of the same terms on
   either side (at scale 0 exact ties between different entries are common); the picked tokens;
   the n_hyp == 0 and all -inf rules.
4. ``encode_and_decode(..., mbr_scale=s)`` for every decoder with an n-best equals ``mbr_select``
   by hand on the n-best in ``info``; ``map_k`` is the result without the keyword; a scale of 1e4
   returns ``map_k`` where the top two totals differ by more than 1e-2; graphed equals eager,
   timestamps included.
5. ``token_error_counts`` / ``compute_wer_device`` equal the host helpers.
"""
import functools
import math
import random

import numpy as np
import pytest
import torch

import ngram_ref as nr
from edit_ref import edit_distance_np, edit_ops, mbr, pairwise

pytestmark = pytest.mark.gpu

LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 200)


def _mutate(rng, seq, alphabet, edits):
    seq = list(seq)
    for _ in range(edits):
        kind = rng.randrange(3)
        pos = rng.randrange(len(seq) + 1)
        if kind == 0 and seq:
            seq[min(pos, len(seq) - 1)] = rng.randrange(alphabet)
        elif kind == 1:
            seq.insert(pos, rng.randrange(alphabet))
        elif seq:
            del seq[min(pos, len(seq) - 1)]
    return seq


@functools.lru_cache(maxsize=None)
def _pairs():
    """[(a, b) or None for an absent pair] and the oracle's (d, sub, ins, del): computed once,
    shared, never modified."""
    rng = random.Random(11)
    pairs = []
    for alphabet in (2, 5004):
        for la in LENGTHS:
            for lb in LENGTHS:
                a = [rng.randrange(alphabet) for _ in range(la)]
                # the hypothesis follows the reference with a few edits, then takes its own length
                b = _mutate(rng, a, alphabet, rng.randrange(6))[:lb]
                b += [rng.randrange(alphabet) for _ in range(lb - len(b))]
                pairs.append((tuple(a), tuple(b)))
    for n in (1, 64, 65, 200):                                     # identical pairs
        a = tuple(rng.randrange(3) for _ in range(n))
        pairs.append((a, a))
    pairs.insert(7, None)                                          # absent pairs
    pairs.append(None)
    want = [(-1, -1, -1, -1) if p is None else edit_ops(*p) for p in pairs]
    return tuple(pairs), tuple(want)


def _padded(seqs, width, fill_rng, absent_len=-1):
    """[P, width] int64 and lengths; the padding holds live-looking tokens."""
    out = torch.tensor([[fill_rng.randrange(2) for _ in range(width)] for _ in seqs],
                       dtype=torch.int64).reshape(len(seqs), width)
    lens = []
    for k, s in enumerate(seqs):
        if s is None:
            lens.append(absent_len)
            continue
        out[k, :len(s)] = torch.tensor(s, dtype=torch.int64)
        lens.append(len(s))
    return out, torch.tensor(lens, dtype=torch.int32)


@pytest.mark.parametrize("slack", [(0, 0), (30, 17)], ids=["tight", "slack"])
def test_edit_distance_matches_oracle(gpu, slack):
    from onebit_asr.edit import edit_distance

    pairs, want = _pairs()
    rng = random.Random(3)
    a, a_len = _padded([p and p[0] for p in pairs], max(LENGTHS) + slack[0], rng)
    b, b_len = _padded([p and p[1] for p in pairs], max(LENGTHS) + slack[1], rng, absent_len=5)
    a_len[-1], b_len[-1] = 7, -3                                   # absent on either side
    dist, ops = edit_distance(a.to(gpu), a_len.to(gpu), b.to(gpu), b_len.to(gpu), ops=True)
    only = edit_distance(a.to(gpu).int(), a_len.to(gpu), b.to(gpu).int(), b_len.to(gpu))
    assert dist.dtype == ops.dtype == only.dtype == torch.int32 and ops.shape == (len(pairs), 3)
    got = torch.cat([dist[:, None], ops], dim=1).cpu().tolist()
    bad = [(k, g, w) for k, (g, w) in enumerate(zip(got, want)) if tuple(g) != w]
    assert not bad, bad[:5]
    assert only.cpu().tolist() == [w[0] for w in want]             # the distance-only kernel
    if slack != (0, 0):
        # lengths above the width are clamped to it
        big = torch.full_like(a_len, 10 ** 6)
        clamped = edit_distance(a.to(gpu), big.to(gpu), b.to(gpu), big.to(gpu))
        k = 5
        assert int(clamped[k]) == edit_distance_np(a[k].tolist(), b[k].tolist())


def test_edit_distance_at_the_length_limit(gpu):
    from onebit_asr.edit import edit_distance

    rs = np.random.RandomState(4)
    a, b = rs.randint(0, 4, size=4096), rs.randint(0, 4, size=4000)
    a_t = torch.from_numpy(a)[None].to(gpu)
    b_t = torch.cat([torch.from_numpy(b), torch.zeros(96, dtype=torch.int64)])[None].to(gpu)
    dist = edit_distance(a_t, torch.tensor([4096], device=gpu), b_t,
                         torch.tensor([4000], device=gpu))
    want = edit_distance_np(a.tolist(), b)
    assert dist.cpu().tolist() == [want]
    # the same pair with the counts, which add up; and an unsupported width
    d2, ops = edit_distance(a_t, torch.tensor([4096], device=gpu), b_t,
                            torch.tensor([4000], device=gpu), ops=True)
    sub, ins, dele = ops[0].cpu().tolist()
    assert int(d2) == want == sub + ins + dele and ins - dele == 4000 - 4096
    with pytest.raises(ValueError, match="not supported"):
        edit_distance(torch.zeros(1, 4097, dtype=torch.int32, device=gpu),
                      torch.tensor([1], device=gpu), b_t, torch.tensor([1], device=gpu))
    empty = edit_distance(a_t[:0], torch.zeros(0, device=gpu), b_t[:0], torch.zeros(0, device=gpu))
    assert empty.shape == (0,)


# ------------------------------------------------------------------------------------------
# n-best
# ------------------------------------------------------------------------------------------
B, T, S = 4, 40, 36


@functools.lru_cache(maxsize=None)
def _nbest(N, seed=0):
    """An n-best of B utterances: entries are 0 to 4 random edits of a base sequence, n_hyp in
    {0, 1, N}; with the reference and the oracle's dref / ops / dpair."""
    rng = random.Random(100 * N + seed)
    n_hyp = [N, 0, 1, N]
    entries, refs = [], []
    for b in range(B):
        base = [rng.randrange(4, 30) for _ in range(rng.randint(8, 30))]
        refs.append(tuple(_mutate(rng, base, 30, rng.randrange(3))[:S]))
        entries.append(tuple(tuple(_mutate(rng, base, 30, rng.randrange(5))[:T])
                             for _ in range(N)))
    dref = [[edit_ops(refs[b], entries[b][k]) if k < n_hyp[b] else (-1,) * 4 for k in range(N)]
            for b in range(B)]
    dpair = [pairwise(entries[b], n_hyp[b], N) for b in range(B)]
    return tuple(entries), tuple(refs), tuple(n_hyp), dref, dpair


def _nbest_tensors(N, gpu, seed=0):
    entries, refs, n_hyp, _, _ = _nbest(N, seed)
    rng = random.Random(1)
    hyp = torch.tensor([[[rng.randrange(4, 30) for _ in range(T)] for _ in range(N)]
                        for _ in range(B)], dtype=torch.int32)
    hyp_len = torch.zeros(B, N, dtype=torch.int32)
    for b in range(B):
        for k in range(N):
            e = entries[b][k]
            hyp[b, k, :len(e)] = torch.tensor(e, dtype=torch.int32)
            hyp_len[b, k] = len(e)   # absent entries keep a live-looking length and tokens
    ref, ref_len = _padded(refs, S, rng)
    return (hyp.to(gpu), hyp_len.to(gpu), torch.tensor(n_hyp, dtype=torch.int32, device=gpu),
            ref.to(gpu), ref_len.to(gpu))


@pytest.mark.parametrize("N", [1, 5, 32])
def test_nbest_edit_distance_matches_oracle(gpu, N):
    from onebit_asr.edit import edit_distance, nbest_edit_distance, nbest_oracle

    _, _, n_hyp, want_ref, want_pair = _nbest(N)
    hyp, hyp_len, nh, ref, ref_len = _nbest_tensors(N, gpu)
    res = nbest_edit_distance(hyp, hyp_len, nh, ref, ref_len, pairwise=True)
    assert set(res) == {"dref", "ops", "dpair"}
    assert all(v.dtype == torch.int32 and v.is_cuda for v in res.values())
    got = torch.cat([res["dref"][..., None], res["ops"]], dim=-1).cpu().tolist()
    assert got == [[list(c) for c in row] for row in want_ref]
    dpair = res["dpair"].cpu()
    assert dpair.tolist() == want_pair
    assert torch.equal(dpair, dpair.transpose(1, 2))
    for b in range(B):
        n = n_hyp[b]
        assert (torch.diagonal(dpair[b])[:n] == 0).all()
        assert (dpair[b, n:] == -1).all() and (dpair[b, :, n:] == -1).all()
        assert (dpair[b, :n, :n] >= 0).all()
    # each output on its own is the same bits
    only_pair = nbest_edit_distance(hyp, hyp_len, nh, pairwise=True)
    only_ref = nbest_edit_distance(hyp, hyp_len, nh, ref, ref_len)
    assert set(only_pair) == {"dpair"} and set(only_ref) == {"dref", "ops"}
    assert torch.equal(only_pair["dpair"], res["dpair"])
    assert torch.equal(only_ref["dref"], res["dref"]) and torch.equal(only_ref["ops"], res["ops"])
    # the per-pair call on the live entries, bit for bit
    live = torch.arange(N, device=gpu)[None, :] < nh[:, None]
    pair_len = torch.where(live, hyp_len, torch.full_like(hyp_len, -1)).reshape(-1)
    d, ops = edit_distance(ref.repeat_interleave(N, dim=0), ref_len.repeat_interleave(N),
                           hyp.reshape(B * N, T), pair_len, ops=True)
    assert torch.equal(d.reshape(B, N), res["dref"])
    assert torch.equal(ops.reshape(B, N, 3), res["ops"])
    # the oracle entry
    best_k, dist = nbest_oracle(res["dref"])
    for b in range(B):
        ds = [want_ref[b][k][0] for k in range(n_hyp[b])]
        assert (int(best_k[b]), int(dist[b])) == ((ds.index(min(ds)), min(ds)) if ds else (0, -1))
    with pytest.raises(ValueError, match="nothing to compute"):
        nbest_edit_distance(hyp, hyp_len, nh)
    with pytest.raises(ValueError, match="go together"):
        nbest_edit_distance(hyp, hyp_len, nh, ref)


# ------------------------------------------------------------------------------------------
# MBR
# ------------------------------------------------------------------------------------------
SEEDS = 4


def _scores(N, seed):
    """Descending normal scores per utterance, float64 [B, N]."""
    rs = np.random.RandomState(500 + 10 * N + seed)
    return -np.sort(-rs.standard_normal((B, N)) * 2.0, axis=1)


@pytest.mark.parametrize("N", [2, 5, 10, 32])
@pytest.mark.parametrize("scale", [0.0, 0.5, 1.0])
def test_mbr_select_matches_oracle(gpu, N, scale):
    from onebit_asr.edit import mbr_select

    for seed in range(SEEDS):
        entries, _, n_hyp, _, want_pair = _nbest(N, seed)
        hyp, hyp_len, nh, _, _ = _nbest_tensors(N, gpu, seed)
        scores = _scores(N, seed)
        out, cnt, info = mbr_select(hyp, hyp_len, nh, torch.from_numpy(scores).to(gpu), scale)
        assert set(info) == {"best_k", "risk", "post", "dpair"}
        assert info["risk"].dtype == info["post"].dtype == torch.float64
        assert out.dtype == cnt.dtype == info["best_k"].dtype == torch.int32
        assert info["dpair"].cpu().tolist() == want_pair
        risk, post = info["risk"].cpu().numpy(), info["post"].cpu().numpy()
        for b in range(B):                                          # no utterance is skipped
            k_ref, risk_ref, post_ref = mbr(want_pair[b], scores[b].tolist(), n_hyp[b], scale)
            n = n_hyp[b]
            if n:
                worst = np.abs(risk[b, :n] - risk_ref[:n]).max() / max(max(risk_ref[:n]), 1e-300)
                print(f"N {N} scale {scale} seed {seed} b {b}: risk off by {worst:.2e} (relative)")
            np.testing.assert_allclose(post[b], post_ref, rtol=1e-11, atol=0)
            np.testing.assert_allclose(risk[b], risk_ref, rtol=1e-11, atol=0)
            k = int(info["best_k"][b])
            if n == 0:
                assert (k, int(cnt[b])) == (0, 0) and (out[b] == -1).all()
                continue
            assert 0 <= k < n and risk_ref[k] <= min(risk_ref[:n]) + 1e-9
            if scale > 0:
                assert k == k_ref
            e = entries[b][k]
            assert int(cnt[b]) == len(e) and out[b, :len(e)].tolist() == list(e)
            assert (out[b, len(e):] == -1).all()


def test_mbr_select_rules(gpu):
    from onebit_asr.edit import mbr_select

    N = 5
    hyp, hyp_len, nh, _, _ = _nbest_tensors(N, gpu)
    ninf = -math.inf
    scores = torch.tensor([[ninf] * N,                 # a rescore utterance that was not rescored
                           [0.0] * N,                  # n_hyp == 0
                           [-1.0] * N,
                           [ninf, -2.0, -1.0, ninf, -3.0]], dtype=torch.float64, device=gpu)
    out, cnt, info = mbr_select(hyp, hyp_len, nh, scores, 1.0)
    risk, post = info["risk"].cpu(), info["post"].cpu()
    assert info["best_k"][:2].tolist() == [0, 0]
    assert torch.isinf(risk[0]).all() and (post[0] == 0).all()
    assert int(cnt[0]) == int(hyp_len[0, 0]) and torch.equal(out[0, :cnt[0]], hyp[0, 0, :cnt[0]])
    assert int(cnt[1]) == 0 and (out[1] == -1).all()
    assert torch.isinf(risk[1]).all() and (post[1] == 0).all()
    assert post[2].tolist() == [1.0, 0, 0, 0, 0] and risk[2, 0] == 0 and torch.isinf(risk[2, 1:]).all()
    # entries at -inf weigh nothing but still have a risk
    _, _, _, _, want_pair = _nbest(N)
    k_ref, risk_ref, post_ref = mbr(want_pair[3], scores[3].tolist(), N, 1.0)
    assert post[3, 0] == 0 and post[3, 3] == 0 and int(info["best_k"][3]) == k_ref
    np.testing.assert_allclose(risk[3].numpy(), risk_ref, rtol=1e-11)
    np.testing.assert_allclose(post[3].numpy(), post_ref, rtol=1e-11)
    # float32 scores are taken as they are; a bad scale is refused
    a = mbr_select(hyp, hyp_len, nh, scores.float(), 0.5)[2]
    b = mbr_select(hyp, hyp_len, nh, scores.float().double(), 0.5)[2]
    assert torch.equal(a["best_k"], b["best_k"])
    with pytest.raises(ValueError, match="mbr_scale"):
        mbr_select(hyp, hyp_len, nh, scores, -1.0)


# ------------------------------------------------------------------------------------------
# encode_and_decode / GraphedInference
# ------------------------------------------------------------------------------------------
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


def _same(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape
    assert a.contiguous().view(torch.uint8).equal(b.contiguous().view(torch.uint8))


#            id              decoder      keywords                         the totals in info
CONFIGS = [("beam", "beam", {}, "ctc_scores"),
           ("beam-lm", "beam", dict(lm_weight=0.4), "total"),
           ("beam-lm-first-pass", "beam", dict(lm_weight=0.4, lm_fusion="first_pass",
                                               ins_bonus=0.5), "total"),
           ("rescore", "rescore", dict(max_len=24), "total"),
           ("attention", "attention", dict(max_len=12), "score"),
           ("joint", "attention", dict(max_len=12, joint_ctc_weight=0.3), "score")]


@pytest.mark.parametrize("name,decoder,kw,totals", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_mbr_scale_in_encode_and_decode_and_graphed(gpu, name, decoder, kw, totals):
    from onebit_asr.edit import mbr_select
    from onebit_asr.infer import GraphedInference, encode_and_decode
    from onebit_asr.quant import set_act_quant

    model, (b1, b2), lm = _model()
    kw = dict(kw, decoder=decoder, beam_size=4)
    if "lm_weight" in kw:
        kw["lm"] = lm
    set_act_quant(model, None)
    keys = ("hyp", "hyp_len", "n_hyp", totals, "best_k", "map_k", "mbr_risk", "mbr_post")
    eager = []
    for b in (b1, b2):
        plain = encode_and_decode(model, b, **kw)
        for scale in (0.7, 1e4):
            info = {}
            out, cnt, logits = encode_and_decode(model, b, info=info, mbr_scale=scale, **kw)
            assert set(info) >= set(keys)
            _same(logits, plain[2])
            # mbr_select by hand on the n-best in info, bit for bit
            h_out, h_cnt, h = mbr_select(info["hyp"], info["hyp_len"], info["n_hyp"],
                                         info[totals], scale)
            _same(out, h_out)
            _same(cnt, h_cnt)
            for x, y in (("best_k", "best_k"), ("mbr_risk", "risk"), ("mbr_post", "post")):
                _same(info[x], h[y])
            # map_k is the entry the decoder returns without the keyword
            for u in range(2):
                k = int(info["map_k"][u])
                n = int(info["hyp_len"][u, k]) if int(info["n_hyp"][u]) > 0 else 0
                assert int(plain[1][u]) == n
                assert plain[0][u, :n].tolist() == info["hyp"][u, k, :n].tolist()
                if scale == 1e4 and int(info["n_hyp"][u]) > 0:
                    top = torch.sort(info[totals][u, :int(info["n_hyp"][u])], descending=True)[0]
                    if len(top) < 2 or (math.isfinite(float(top[0])) and top[0] - top[1] > 1e-2):
                        assert int(info["best_k"][u]) == k
            if scale == 0.7:
                eager.append((out, cnt, {k: info[k] for k in keys}))
    # graphed == eager, with the forced alignment of the MBR output in the graph
    gi = GraphedInference(model, act_quant=None, timestamps=True, mbr_scale=0.7,
                          **{k: v for k, v in kw.items()})
    runs = []
    for b in (b1, b2, b1):
        out, cnt, _ = gi.run(b)
        runs.append((out.clone(), cnt.clone(), {k: gi.info[k].clone() for k in keys},
                     gi.info["span"].clone(), gi.info["align_score"].clone()))
    assert gi.graph is not None
    set_act_quant(model, None)
    for run, want in zip(runs, (eager[0], eager[1], eager[0])):
        _same(run[0], want[0])
        _same(run[1], want[1])
        for k in keys:
            _same(run[2][k], want[2][k])
    # the alignment is that of the MBR output
    info = {}
    out, cnt, _ = encode_and_decode(model, b2, info=info, mbr_scale=0.7, timestamps=True, **kw)
    _same(out, runs[1][0])
    _same(info["span"], runs[1][3])
    _same(info["align_score"], runs[1][4])


def test_greedy_has_no_nbest(gpu):
    from onebit_asr.infer import encode_and_decode

    model, (b1, _), _ = _model()
    with pytest.raises(ValueError, match="mbr_scale needs decoder"):
        encode_and_decode(model, b1, mbr_scale=1.0)


# ------------------------------------------------------------------------------------------
# metrics
# ------------------------------------------------------------------------------------------
def test_token_error_counts_and_compute_wer_device_equal_the_host_helpers(gpu):
    from onebit_asr.metrics import (compute_wer, compute_wer_device, levenshtein_distance,
                                    token_error_counts)

    rng = random.Random(9)
    words = ["the", "a", "cat", "dog", "sat", "on", "mat", "ran", "far", "away", "é", "naïve"]
    refs = [" ".join(rng.choice(words) for _ in range(rng.randint(0, 90))) for _ in range(40)]
    hyps = [" ".join(_mutate(rng, r.split(), 1, 0) if rng.random() < 0.2 else
                     [w for w in r.split() if rng.random() < 0.85] +
                     [rng.choice(words) for _ in range(rng.randrange(3))]) for r in refs]
    assert compute_wer_device(refs, hyps, gpu) == compute_wer(refs, hyps)
    assert compute_wer_device(refs[:1], hyps[:1], gpu) == compute_wer(refs[:1], hyps[:1])
    assert compute_wer_device(["", "a b"], ["a", ""], gpu) == compute_wer(["", "a b"], ["a", ""])

    pairs, want = _pairs()
    live = [(p, w) for p, w in zip(pairs, want) if p is not None][::7]
    ref, ref_len = _padded([p[0] for p, _ in live], max(LENGTHS) + 3, rng)
    hyp, cnt = _padded([p[1] for p, _ in live], max(LENGTHS), rng)
    got = token_error_counts(hyp.to(gpu), cnt.to(gpu), ref.to(gpu), ref_len.to(gpu))
    assert set(got) == {"dist", "sub", "ins", "del", "ref_tokens"}
    assert all(v.dtype == torch.int64 and v.is_cuda and v.dim() == 0 for v in got.values())
    assert int(got["dist"]) == sum(levenshtein_distance(p[0], p[1]) for p, _ in live)
    for k, name in enumerate(("dist", "sub", "ins", "del")):
        assert int(got[name]) == sum(w[k] for _, w in live), name
    assert int(got["ref_tokens"]) == sum(len(p[0]) for p, _ in live)
    # an absent pair is left out of every total
    k = max(range(len(live)), key=lambda i: live[i][1][0])
    cnt2 = cnt.clone()
    cnt2[k] = -1
    got2 = token_error_counts(hyp.to(gpu), cnt2.to(gpu), ref.to(gpu), ref_len.to(gpu))
    assert live[k][1][0] > 0
    assert int(got2["dist"]) == int(got["dist"]) - live[k][1][0]
    assert int(got2["ref_tokens"]) == int(got["ref_tokens"]) - len(live[k][0][0])
