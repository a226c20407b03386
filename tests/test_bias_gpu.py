"""GPU: phrase-list contextual biasing on the device (csrc/bias.hip, the biased searches of
csrc/beam.hip and csrc/attdec.hip) against the oracle of tests/bias_ref.py.

The bias term is a float64 sum of float32 node values in a fixed order: it is compared bit for bit,
with the oracle and with the library's host walker. The CTC search follows test_beam_lm_gpu.py's
rule: both sides are fp64 from the same fp32 logits, ``ctc`` agrees to 1e-9 * max(1, T), and where
the oracle's smallest decision margin is >= 1e-6 the hypotheses are exactly the oracle's; ``total``
is bit for bit its formula over the device's own outputs. The beam step is driven with the
oracle's candidates and compared exactly, as test_ngram_gpu.py drives the fused step.
"""
import functools
import math

import numpy as np
import pytest
import torch

import attdec_ref as ar
import bias_ref as br
import joint_ref as jr
import ngram_ref as nr
import test_joint_gpu as tj
from ctc_beam_ref import beam_search, ctc_like_logits, ragged_lens

pytestmark = pytest.mark.gpu

NEG_INF = -math.inf
PAD, BOS, EOS, BLANK = 0, 1, 2, 3
MARGIN = 1e-6
NK = [(1, 1), (4, 8), (10, 20)]


def _bits(x):
    return np.asarray(x, np.float64).view(np.int64)


def _bytes(t):
    return t.cpu().numpy().tobytes()


def _ctx(phrases, boost=1.0):
    from onebit_asr.bias import ContextBias

    return ContextBias(phrases, boost)


# ------------------------------------------------------------------------------------------
# 1. the scorers
# ------------------------------------------------------------------------------------------
# four token groups, one per branch family of the step: the fail link (10 11 10 | 11), a finished
# phrase with a longer one behind it (commit, restart), a finished phrase on the fail path
# (30 31 32 | x), a single-token phrase
STEP_PHRASES = [([10, 11, 10, 12], 1.0), ([20, 21], 1.0), ([20, 21, 22], 3.0),
                ([30, 31, 32, 33], 1.7), ([31, 32], 2.3), ([25], 2.5)]
POOL = [10, 11, 12, 20, 21, 22, 30, 31, 32, 33, 25, 5, 6]
SCRIPT = [30, 31, 32, 5, 10, 11, 10, 11]      # row 0's tokens: the two fail-link branches for sure
ALL_TAGS = {"edge", "edge_after_fail", "commit", "commit_on_fail_path", "restart_hit",
            "restart_miss", "root_miss", "leaf"}


def _next_token(ref, toks, rng):
    """A token that continues the prefix's match (most of the time) or any pool token."""
    state = ref.walk(toks)[0]
    kids = [p[-1] for p in ref.nodes if len(p) == len(state) + 1 and p[:-1] == state]
    if kids and rng.random() < 0.65:
        return int(kids[int(rng.integers(len(kids)))])
    return int(POOL[int(rng.integers(len(POOL)))])


@pytest.mark.parametrize("N,K", NK, ids=[f"N{n}-K{k}" for n, k in NK])
def test_bias_step_equals_the_oracle_bit_for_bit(gpu, N, K):
    from onebit_asr.bias import bias_step

    ref, ctx = br.RefBias(STEP_PHRASES), _ctx(STEP_PHRASES)
    num = br.node_numbers(ref)
    rng = np.random.default_rng(100 * N + K)
    B, steps = 3, 9
    R = B * N
    st = torch.full((2, R), 0, dtype=torch.int32, device=gpu)
    kept = torch.full((2, R), 77.0, dtype=torch.float64, device=gpu)
    prev = [None] * R                 # the prefix whose pair the last table holds, per row
    tags, kinds = set(), set()
    for s in range(steps):
        live_prev = [r for r in range(R) if prev[r] is not None]
        cur = [None] * R
        tok = np.full(R, 12345, np.int64)
        length = np.full(R, 9, np.int32)
        link = np.full((R, 2), 12345, np.int32)
        skip = np.zeros(R, np.uint8)
        for r in range(R):
            u = rng.random()
            if r == 0 and s > 0:
                w = SCRIPT[s - 1]
                cur[r], length[r], tok[r] = prev[0] + [w], s, w
                link[r] = (0, -1)
                kinds.add("extend")
            elif s > 0 and u < 0.15:
                skip[r] = 1
                kinds.add("skip")
            elif s == 0 or u < 0.22:
                cur[r], length[r], tok[r] = [], 0, BOS
                kinds.add("len0")
            elif u < 0.32 or not live_prev:
                w = _next_token(ref, [], rng)
                cur[r], length[r], tok[r] = [w], 1, w           # the link is not read
                kinds.add("len1")
            else:
                p = live_prev[int(rng.integers(len(live_prev)))]
                w = _next_token(ref, prev[p], rng)
                cur[r], length[r], tok[r] = prev[p] + [w], len(prev[p]) + 1, w
                link[r] = (p, -1)
                kinds.add("extend")
        topi = np.full((R, K), -1, np.int32)
        for r in range(R):
            if cur[r] is None:
                topi[r] = 4242                                   # never read
                continue
            n_c = K if rng.random() < 0.5 else int(rng.integers(0, K + 1))
            cands = [_next_token(ref, cur[r], rng) for _ in range(n_c)]
            if cands and rng.random() < 0.6:
                cands[int(rng.integers(len(cands)))] = EOS
            topi[r, :n_c] = cands
        bsc = torch.full((R, K), 77.0, dtype=torch.float64, device=gpu)
        i, o = s & 1, (s + 1) & 1
        before_st, before_kept = st[o].clone(), kept[o].clone()
        bias_step(ctx, torch.from_numpy(topi).to(gpu), torch.from_numpy(tok).to(gpu),
                  torch.from_numpy(length).to(gpu), torch.from_numpy(link).to(gpu),
                  torch.from_numpy(skip).to(gpu), st[i], st[o], kept[i], kept[o], bsc, N, EOS)
        g_st, g_kept, g_bsc = st[o].cpu().numpy(), kept[o].cpu().numpy(), bsc.cpu().numpy()
        for r in range(R):
            if cur[r] is None:
                assert g_st[r] == before_st[r].item() and \
                    _bits(g_kept[r]) == _bits(before_kept[r].item()), (s, r)
                assert (g_bsc[r] == 77.0).all(), (s, r)
                continue
            state, k0, _, fin = ref.walk(cur[r], tags)
            assert g_st[r] == num[state] and _bits(g_kept[r]) == _bits(k0), (s, r, cur[r])
            for q in range(K):
                c = int(topi[r, q])
                if c < 0:
                    want = NEG_INF
                    kinds.add("absent")
                elif c == EOS:
                    want = fin
                    kinds.add("eos")
                else:
                    s2, k2 = ref.step(state, k0, c, tags)
                    want = k2 + ref.phi(s2)
                assert _bits(g_bsc[r, q]) == _bits(want), (s, r, q, cur[r], c)
        prev = cur
    assert {"len0", "extend"} <= kinds
    if N > 1:
        assert kinds == {"len0", "len1", "extend", "skip", "absent", "eos"}
        assert tags == ALL_TAGS, ALL_TAGS - tags


@pytest.mark.parametrize("T", [1, 7, 61])
def test_bias_seq_score_equals_the_oracle_bit_for_bit(gpu, T):
    from onebit_asr.bias import bias_seq_score

    ref, ctx = br.RefBias(STEP_PHRASES), _ctx(STEP_PHRASES)
    rng = np.random.default_rng(T)
    rows = 70                                            # more than one block of 64 rows
    hyp = np.full((2, rows // 2, T), -1, np.int32)
    lens = np.zeros((2, rows // 2), np.int32)
    for a in range(2):
        for r in range(rows // 2):
            n = int(rng.integers(0, T + 1))
            toks = []
            while len(toks) < n:
                toks.append(_next_token(ref, toks, rng))
            hyp[a, r, :n] = toks
            lens[a, r] = n if rng.random() < 0.9 else -1   # an absent row
    lens[0, 0], lens[1, 0] = 0, T
    got = bias_seq_score(ctx, torch.from_numpy(hyp).to(gpu), torch.from_numpy(lens).to(gpu))
    assert got.shape == (2, rows // 2) and got.dtype == torch.float64
    got = got.cpu().numpy()
    for a in range(2):
        for r in range(rows // 2):
            n = lens[a, r]
            want = NEG_INF if n < 0 else ref.bias_fin(hyp[a, r, :n].tolist())
            assert _bits(got[a, r]) == _bits(want), (a, r)
            if n >= 0:
                assert _bits(ctx.bias_fin(hyp[a, r, :n].tolist())) == _bits(want)
    assert (got > 0).any() and (got == NEG_INF).any()


# ------------------------------------------------------------------------------------------
# 2. the biased CTC prefix beam search
# ------------------------------------------------------------------------------------------
#         B   T    V   beam top_k bias_weight boost
CASES = [(1, 1, 5, 10, 20, 1.0, 2.0),
         (3, 17, 7, 10, 20, 0.5, 3.0),
         (4, 64, 40, 10, 20, 1.0, 1.5),
         (2, 16, 5004, 10, 20, 1.0, 2.0),
         (4, 33, 40, 4, 20, 2.0, 1.0),
         (4, 64, 40, 1, 20, 1.0, 2.0),
         (3, 48, 70, 16, 32, 0.7, 2.5),
         (2, 40, 12, 32, 20, 1.0, 1.0)]
IDS = ["-".join(map(str, c)) for c in CASES]
LM_CASE = 2                  # the case that also runs with an LM: order 3, lm_weight 0.3, bonus 0.5
LM_ARGS = (3, 0.3, 0.5)


@functools.lru_cache(maxsize=None)
def _case(i):
    """Inputs, phrase list and the oracle's results of CASES[i] (with and without the bias):
    computed once, shared, never modified."""
    B, T, V, beam, top_k, bw, boost = CASES[i]
    logits = ctc_like_logits(3000 + i, B, T, V, BLANK)
    lens = ragged_lens(3000 + i, B, T)
    logits.setflags(write=False)
    lens.setflags(write=False)
    rng = np.random.default_rng(3000 + i)
    plain = [beam_search(logits[b, :lens[b]], beam, BLANK, top_k) for b in range(B)]
    phrases = []
    for r in plain:                  # spans of the runners-up: what a bias can bring forward
        for entry, mult in zip(r.final_beam[1:4], (0.5, 1.0, 2.0)):
            if entry:
                n = int(rng.integers(1, min(4, len(entry)) + 1))
                s = int(rng.integers(0, len(entry) - n + 1))
                phrases.append((list(entry[s:s + n]), boost * mult))
    for _ in range(12):
        phrases.append(([int(t) for t in rng.integers(4, V, size=int(rng.integers(1, 5)))], boost))
    ref = br.RefBias(phrases)
    refs = br.biased_beam_search_batch(logits, lens, ref, bw, None, 0.0, 0.0, beam, BLANK, top_k)
    return logits, lens, tuple(phrases), ref, tuple(refs), tuple(plain)


@functools.lru_cache(maxsize=None)
def _lm_tables():
    V = CASES[LM_CASE][2]
    entries, ids, n, vals = nr.random_lm(300 + LM_CASE, LM_ARGS[0], V, 40 * V)
    return nr.RefLM(entries, LM_ARGS[0]), (ids, n, vals)


@functools.lru_cache(maxsize=None)
def _lm():
    from onebit_asr.ngram import NGramLM

    ref, (ids, n, vals) = _lm_tables()
    return NGramLM.from_arrays(ids, n, vals, ref.order)


@functools.lru_cache(maxsize=None)
def _lm_case():
    B, T, V, beam, top_k, bw, boost = CASES[LM_CASE]
    logits, lens, phrases, ref, _, _ = _case(LM_CASE)
    _, lw, bonus = LM_ARGS
    return tuple(br.biased_beam_search_batch(logits, lens, ref, bw, _lm_tables()[0], lw, bonus,
                                             beam, BLANK, top_k))


def _device(i, gpu, bw=None, lm=None, lw=0.0, bonus=0.0, nbest=None):
    from onebit_asr.infer import ctc_beam_search_bias_device

    B, T, V, beam, top_k, bw0, _ = CASES[i]
    logits, lens, phrases = _case(i)[:3]
    hyp, hyp_len, n_hyp, info = ctc_beam_search_bias_device(
        torch.from_numpy(np.ascontiguousarray(logits)).to(gpu), torch.from_numpy(lens).to(gpu),
        _ctx(phrases), bw0 if bw is None else bw, lm, lw, bonus, beam_size=beam, nbest=nbest,
        blank_id=BLANK, top_k_per_t=top_k)
    nb = beam if nbest is None else nbest
    assert hyp.dtype == hyp_len.dtype == n_hyp.dtype == torch.int32
    assert hyp.shape == (B, nb, T) and hyp_len.shape == (B, nb) and n_hyp.shape == (B,)
    assert set(info) == {"ctc", "lm", "bias", "total"}
    for v in info.values():
        assert v.dtype == torch.float64 and v.shape == (B, nb) and v.is_cuda
    return (hyp.cpu().numpy(), hyp_len.cpu().numpy(), n_hyp.cpu().numpy(),
            {k: v.cpu().numpy() for k, v in info.items()})


def _tokens(hyp, hyp_len, b, k):
    return hyp[b, k, :hyp_len[b, k]].tolist()


def test_the_cases_meet_their_conditions():
    """From the oracle alone, before anything runs on the device."""
    changed = 0
    for i, (B, T, V, beam, top_k, bw, boost) in enumerate(CASES):
        logits, lens, phrases, ref, refs, plain = _case(i)
        assert lens[0] == T and (B == 1 or lens[-1] == 0)
        assert sum(r.margin < MARGIN for r in refs) <= B // 16, i
        if i in (1, 2, 4, 6, 7):                     # extensions land on live prefixes there
            assert sum(r.merges for r in refs) > 0, i
        changed += any(r.tokens != p.tokens for r, p in zip(refs, plain))
        print(f"case {i}: margins {[f'{r.margin:.2e}' for r in refs]} merges "
              f"{[r.merges for r in refs]} changed "
              f"{[r.tokens != p.tokens for r, p in zip(refs, plain)]}")
    assert changed >= 5, changed
    assert sum(r.margin < MARGIN for r in _lm_case()) == 0
    assert sum(r.merges for r in _lm_case()) > 0


def _check_search(i, refs, got, lw, bonus, lm_host):
    B, T, V, beam, top_k, bw, boost = CASES[i]
    logits, lens, phrases, ref = _case(i)[:4]
    hyp, hyp_len, n_hyp, info = got
    ctx = _ctx(phrases)
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
            toks_k = _tokens(hyp, hyp_len, b, k)
            # bias: the closed value of the entry's own tokens, by the host walker and the oracle
            assert _bits(info["bias"][b, k]) == _bits(ctx.bias_fin(toks_k)), (b, k)
            assert _bits(info["bias"][b, k]) == _bits(ref.bias_fin(toks_k)), (b, k)
            if lm_host is None:
                assert _bits(info["lm"][b, k]) == _bits(0.0), (b, k)
            else:
                assert _bits(info["lm"][b, k]) == _bits(lm_host.seq_logprob(toks_k)), (b, k)
            # total: its formula over the device's own outputs, each operation rounded
            want = ((info["ctc"][b, k] + np.float64(lw) * info["lm"][b, k])
                    + np.float64(bonus) * np.float64(m)) + np.float64(bw) * info["bias"][b, k]
            assert _bits(info["total"][b, k]) == _bits(want), (b, k)
        assert (np.diff(info["total"][b, :n]) <= 0).all(), b
        toks, ctc, lm_fin, b_fin, total = r.beam[0]
        got0 = _tokens(hyp, hyp_len, b, 0)
        err = abs(float(info["ctc"][b, 0]) - ctc)
        print(f"utt {b}: margin {r.margin:.3e} gap {r.gap:.3e} merges {r.merges} ctc err "
              f"{err:.3e} n {len(got0)} ref n {len(toks)} bias {b_fin}")
        if r.margin < MARGIN:
            low += 1
            assert got0 in r.final_beam, (b, got0)
            continue
        assert got0 == toks, (b, got0, toks)
        assert err <= 1e-9 * max(1, T), (b, float(info["ctc"][b, 0]), ctc)
        assert _bits(info["bias"][b, 0]) == _bits(b_fin), (b, float(info["bias"][b, 0]), b_fin)
        assert _bits(info["lm"][b, 0]) == _bits(lm_fin), b
        if lens[b] == 0:
            assert got0 == [] and n == 1 and info["ctc"][b, 0] == 0.0
            assert _bits(info["bias"][b, 0]) == _bits(0.0)
        if r.gap >= MARGIN:     # every adjacent pair of totals is apart: the whole order
            assert [_tokens(hyp, hyp_len, b, k) for k in range(n)] == r.final_beam, b
            for k, (_, c_k, l_k, b_k, _) in enumerate(r.beam):
                assert abs(float(info["ctc"][b, k]) - c_k) <= 1e-9 * max(1, T), (b, k)
                assert _bits(info["lm"][b, k]) == _bits(l_k), (b, k)
                assert _bits(info["bias"][b, k]) == _bits(b_k), (b, k)
    assert low <= B // 16


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_biased_search_matches_oracle(gpu, i):
    refs = _case(i)[4]
    assert sum(r.margin < MARGIN for r in refs) <= CASES[i][0] // 16
    _check_search(i, refs, _device(i, gpu), 0.0, 0.0, None)


def test_biased_search_with_an_lm_matches_oracle(gpu):
    order, lw, bonus = LM_ARGS
    refs = _lm_case()
    assert any(r.tokens != p.tokens for r, p in zip(refs, _case(LM_CASE)[4]))   # the LM matters
    _check_search(LM_CASE, refs, _device(LM_CASE, gpu, lm=_lm(), lw=lw, bonus=bonus), lw, bonus,
                  _lm())


@pytest.mark.parametrize("i", [2, 6, 7], ids=[IDS[2], IDS[6], IDS[7]])
def test_weight_zero_is_the_lm_search_and_the_plain_nbest_bit_for_bit(gpu, i):
    from onebit_asr.infer import ctc_beam_search_lm_device, ctc_beam_search_nbest_device
    from onebit_asr.ngram import NGramLM

    B, T, V, beam, top_k = CASES[i][:5]
    logits, lens = _case(i)[:2]
    x = torch.from_numpy(np.ascontiguousarray(logits)).to(gpu)
    ln = torch.from_numpy(lens).to(gpu)
    # no LM, no bonus: the plain n-best
    hyp, hyp_len, n_hyp, info = _device(i, gpu, bw=0.0)
    p_hyp, p_len, p_n, p_score = ctc_beam_search_nbest_device(x, ln, beam_size=beam,
                                                              blank_id=BLANK, top_k_per_t=top_k)
    assert (hyp == p_hyp.cpu().numpy()).all() and (hyp_len == p_len.cpu().numpy()).all()
    assert (n_hyp == p_n.cpu().numpy()).all()
    assert (_bits(info["ctc"]) == _bits(p_score.cpu().numpy())).all()
    assert (_bits(info["total"]) == _bits(p_score.cpu().numpy())).all()
    live = np.arange(beam)[None, :] < n_hyp[:, None]
    assert (info["lm"][live] == 0.0).all() and (info["lm"][~live] == -np.inf).all()
    # with an LM and a bonus: the fused search
    entries, ids, n, vals = nr.random_lm(300 + i, 3, V, 40 * V)
    lm = NGramLM.from_arrays(ids, n, vals, 3)
    hyp, hyp_len, n_hyp, info = _device(i, gpu, bw=0.0, lm=lm, lw=0.3, bonus=0.5)
    l_hyp, l_len, l_n, l_info = ctc_beam_search_lm_device(x, ln, lm, 0.3, 0.5, beam_size=beam,
                                                          blank_id=BLANK, top_k_per_t=top_k)
    assert (hyp == l_hyp.cpu().numpy()).all() and (hyp_len == l_len.cpu().numpy()).all()
    assert (n_hyp == l_n.cpu().numpy()).all()
    for key in ("ctc", "lm", "total"):
        assert (_bits(info[key]) == _bits(l_info[key].cpu().numpy())).all(), key


# ------------------------------------------------------------------------------------------
# 3. the biased beam step / finalize against the oracle bookkeeping
# ------------------------------------------------------------------------------------------
# boosts that are binary fractions: the sums are exact, as the hash scores of the other terms
BOOK_PHRASES = [([9, 17, 5], 0.5), ([9, 17], 0.25), ([30, 12, 21, 8], 0.75), ([14], 1.5),
                ([6, 7], 1.0), ([7, 6, 7], 0.5), ([22, 23, 24, 25, 26], 0.125)]


class _HashLM:
    """Lm increments of (prefix, token): multiples of 1/64 in [-8, 0] (exact sums)."""

    def __init__(self, seed):
        self.seed = seed

    def score(self, toks, v):
        import zlib

        return -float(zlib.crc32(repr(("lm", self.seed, tuple(toks), int(v))).encode()) % 513) / 64.0


def _run_biased_bookkeeping(gpu, logps, cscores, lms, ref, bw, alive, N, K, L, w, lw, alpha, V):
    from onebit_asr import _lib
    from onebit_asr.attdec import length_norm

    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    banned = {PAD, BOS, BLANK}
    with_lm = lms is not None
    B = len(logps)
    R = B * N
    x0 = np.zeros((1, V))
    refs = [br.biased_search(lp, x0, ref, bw, N, K, L, w, lms[b] if with_lm else None, lw, alpha,
                             alive=a, cscore=cs if w > 0 else None)
            for b, (lp, cs, a) in enumerate(zip(logps, cscores, alive))]
    kmask = torch.zeros(B, 3, dtype=torch.uint8, device=gpu)
    for b, a in enumerate(alive):
        if not a:
            kmask[b] = 1
    f64 = torch.float64
    score = torch.full((B, N), 5.0, dtype=f64, device=gpu)
    att = torch.zeros((B, N), dtype=f64, device=gpu)
    ctc = torch.zeros((B, N), dtype=f64, device=gpu)
    lmst = torch.zeros((B, N), dtype=f64, device=gpu) if with_lm else None
    bst = torch.zeros((B, N), dtype=f64, device=gpu)
    length = torch.full((B, N), 9, dtype=torch.int32, device=gpu)
    fin = torch.full((B, N), 9, dtype=torch.uint8, device=gpu)
    tok = torch.full((R,), 9, dtype=torch.int64, device=gpu)
    skip = torch.full((R,), 9, dtype=torch.uint8, device=gpu)
    link = torch.full((R, 2), 9, dtype=torch.int32, device=gpu)
    anc = torch.full((2, R, L), -5, dtype=torch.int32, device=gpu)
    trp = torch.full((L, B, N), 9, dtype=torch.int32, device=gpu)
    trt = torch.full((L, B, N), 9, dtype=torch.int32, device=gpu)
    trs = torch.full((L, B, N), 9.0, dtype=f64, device=gpu)
    norm = length_norm(L, alpha).to(gpu)
    assert lib.ob_attdec_init(kmask.data_ptr(), B, N, 3, L, BOS, score.data_ptr(),
                              length.data_ptr(), fin.data_ptr(), tok.data_ptr(), skip.data_ptr(),
                              anc[0].data_ptr(), st) == 0
    for t in range(L):
        lse = np.full(R, np.nan)
        topv = np.full((R, K), np.nan, np.float32)
        topi = np.full((R, K), 12345, np.int32)
        cpsi = np.full((R, K), np.nan)
        lmsc = np.full((R, K), np.nan)
        bsc = np.full((R, K), np.nan)
        for b in range(B):
            slots = refs[b].history[t]
            live = [k for k, s in enumerate(slots) if s is not None and not s.fin]
            for k, lp in zip(live, logps[b]([slots[k].toks for k in live])):
                order = jr.top_candidates(lp, banned, K)
                shift = float(b + k)
                r = b * N + k
                lse[r] = shift
                topv[r, :len(order)] = (lp[order] + shift).astype(np.float32)
                topv[r, len(order):] = NEG_INF
                topi[r, :len(order)] = order
                topi[r, len(order):] = -1
                cpsi[r, :len(order)] = [cscores[b](slots[k].toks, v) for v in order]
                cpsi[r, len(order):] = NEG_INF
                if with_lm:
                    lmsc[r, :len(order)] = [lms[b].score(slots[k].toks, v) for v in order]
                    lmsc[r, len(order):] = NEG_INF
                bsc[r, :len(order)] = [ref.bias_fin(slots[k].toks) if v == EOS
                                       else ref.bias(slots[k].toks + [int(v)]) for v in order]
                bsc[r, len(order):] = NEG_INF
        d_lse, d_v, d_i, d_c, d_l, d_b = (torch.from_numpy(a).to(gpu)
                                          for a in (lse, topv, topi, cpsi, lmsc, bsc))
        assert lib.ob_attdec_biased_step(
            d_lse.data_ptr(), d_v.data_ptr(), d_i.data_ptr(), d_c.data_ptr() if w > 0 else None, w,
            d_l.data_ptr() if with_lm else None, lw if with_lm else 0.0, d_b.data_ptr(), bw, B, N,
            K, L, t, EOS, PAD, norm.data_ptr(), anc[t & 1].data_ptr(),
            anc[(t + 1) & 1].data_ptr(), score.data_ptr(), att.data_ptr(), ctc.data_ptr(),
            lmst.data_ptr() if with_lm else None, bst.data_ptr(), length.data_ptr(),
            fin.data_ptr(), tok.data_ptr(), skip.data_ptr(), link.data_ptr(), trp.data_ptr(),
            trt.data_ptr(), trs.data_ptr(), st) == 0
        for b in range(B):
            row = refs[b].trace[t]
            old, new = refs[b].history[t], refs[b].history[t + 1]
            assert trp[t, b].cpu().tolist() == [p for p, _, _ in row], (t, b)
            assert trt[t, b].cpu().tolist() == [v for _, v, _ in row], (t, b)
            assert trs[t, b].cpu().tolist() == [s for _, _, s in row], (t, b)
            inf_or = lambda f: [NEG_INF if s is None else f(s) for s in new]  # noqa: E731
            assert score[b].cpu().tolist() == inf_or(lambda s: s.S)
            assert att[b].cpu().tolist() == inf_or(lambda s: s.A)
            assert ctc[b].cpu().tolist() == inf_or(lambda s: s.C)
            if with_lm:
                assert lmst[b].cpu().tolist() == inf_or(lambda s: s.Lm)
            assert bst[b].cpu().tolist() == inf_or(lambda s: s.Bi)
            assert length[b].cpu().tolist() == [0 if s is None else s.n for s in new]
            assert fin[b].cpu().tolist() == [2 if s is None else int(s.fin) for s in new]
            want_tok = [PAD if (s is None or s.fin) else row[k][1] for k, s in enumerate(new)]
            assert tok[b * N:(b + 1) * N].cpu().tolist() == want_tok
            assert skip[b * N:(b + 1) * N].cpu().tolist() == [0 if (s is not None and not s.fin)
                                                              else 1 for s in new]
            want_link = []
            for k, (p, v, _) in enumerate(row):
                if v >= 0:
                    want_link.append([b * N + p, old[p].toks[-1] if old[p].toks else -1])
                else:
                    want_link.append([b * N + (k if p < 0 else p), -1])
            assert link[b * N:(b + 1) * N].cpu().tolist() == want_link, (t, b)
            want_anc = ar.ancestry(refs[b].trace[:t + 1], N, L, b * N)
            got_anc = anc[(t + 1) & 1, b * N:(b + 1) * N, :t + 1].cpu().tolist()
            assert got_anc == [r_[:t + 1] for r_ in want_anc], (t, b)
    hyp = torch.full((B, N, L), 9, dtype=torch.int32, device=gpu)
    hyp_len = torch.full((B, N), 9, dtype=torch.int32, device=gpu)
    n_hyp = torch.full((B,), 9, dtype=torch.int32, device=gpu)
    out_sc = torch.full((B, N), 9.0, dtype=f64, device=gpu)
    fin_out = torch.full((B, N), 9, dtype=torch.uint8, device=gpu)
    assert lib.ob_attdec_finalize(trp.data_ptr(), trt.data_ptr(), score.data_ptr(),
                                  length.data_ptr(), fin.data_ptr(), B, N, L, EOS,
                                  hyp.data_ptr(), hyp_len.data_ptr(), n_hyp.data_ptr(),
                                  out_sc.data_ptr(), fin_out.data_ptr(), st) == 0
    for b, r in enumerate(refs):
        n = len(r.hyps)
        assert n_hyp[b].item() == n
        for k in range(n):
            m = hyp_len[b, k].item()
            assert hyp[b, k, :m].cpu().tolist() == r.hyps[k]
            assert out_sc[b, k].item() == r.scores[k]
            assert bool(fin_out[b, k].item()) == r.finished[k]
    return refs


@pytest.mark.parametrize("with_lm", [True, False], ids=["lm", "nolm"])
@pytest.mark.parametrize("w", [0.0, 0.25])
@pytest.mark.parametrize("N,K", NK, ids=[f"N{n}-K{k}" for n, k in NK])
def test_biased_step_and_finalize_match_the_oracle(gpu, N, K, w, with_lm):
    V, L, bw, lw = 40, 6, 2.0, 0.5
    ref = br.RefBias(BOOK_PHRASES)
    logps = [jr.hash_logp(100 * N + u, V, EOS) for u in range(4)]
    cs = [tj._hash_cscore(7 * N + u) for u in range(4)]
    lms = [_HashLM(3 * N + u) for u in range(4)] if with_lm else None
    alive = [True, True, False, True]
    refs = _run_biased_bookkeeping(gpu, logps, cs, lms, ref, bw, alive, N, K, L, w, lw, 0.6, V)
    assert refs[2].hyps == []
    assert (sum(r.dropped for r in refs) > 0) == (w > 0)
    if K > 1:       # the bias term matters: the search without it ends elsewhere, and it is used
        none = [br.biased_search(lp, np.zeros((1, V)), ref, 0.0, N, K, L, w,
                                 lms[b] if with_lm else None, lw, 0.6, alive=a,
                                 cscore=c if w > 0 else None)
                for b, (lp, c, a) in enumerate(zip(logps, cs, alive))]
        assert [r.hyps for r in none] != [r.hyps for r in refs]
        assert any(v > 0 for r in refs for v in r.bias)


# ------------------------------------------------------------------------------------------
# 4. end to end on the small synthetic model, and forcing
# ------------------------------------------------------------------------------------------
E2E_PHRASES = [([9, 17, 5], 1.5), ([9, 17], 0.7), ([30, 12], 2.3), ([21], 1.1), ([8, 8, 14], 0.9),
               ([5, 30, 12, 21], 1.3)]
E2E = [(N, L, w, with_lm) for N, L in ((1, 12), (4, 8), (10, 12)) for w, with_lm in
       ((0.0, False), (0.3, False), (0.3, True))]


@functools.lru_cache(maxsize=None)
def _small_lm():
    from onebit_asr.ngram import NGramLM

    entries, ids, n, vals = nr.random_lm(35, 3, 35, 600)
    return NGramLM.from_arrays(ids, n, vals, 3), nr.RefLM(entries, 3)


@pytest.mark.parametrize("N,L,w,with_lm", E2E,
                         ids=[f"N{N}-L{L}-w{w}-{'lm' if m else 'nolm'}" for N, L, w, m in E2E])
def test_biased_joint_search_end_to_end_v35(gpu, N, L, w, with_lm):
    """V = 35, T' in {61, 20, 1}, K = 32 (every unbanned id is a candidate). Along the device's own
    path the bias term is exact: bias_fin of a finished hypothesis, bias of a running one, bit for
    bit by the host walker and the oracle, and score is its formula over the device's own terms.
    The whole search equals the oracle's on the float64 model where the oracle's margin is decisive:
    >= 10 e, e = 4 x the existing fp32 attention path's largest error of A over the prefixes the
    oracle selects at any step + 1e-9 * max(1, T), test_ngram_gpu.py's bound (the bias and LM
    terms are exact and add none)."""
    from onebit_asr.attdec import joint_beam_search

    model, model64 = tj._decoder_model(35, 64)
    enc, mask = tj._memory(0, 64, tj.LENS, gpu)
    lm, ref_lm = _small_lm() if with_lm else (None, None)
    lw, bw, K = (0.5 if with_lm else 0.0), 1.0, 32
    ref, ctx = br.RefBias(E2E_PHRASES), _ctx(E2E_PHRASES)
    B = enc.shape[0]
    with torch.no_grad():
        z = model.ctc_logits(enc).float().contiguous()
    hyp, hyp_len, n_hyp, score, info = joint_beam_search(model, enc, mask, z, N, L, w, K, 0.0,
                                                         lm=lm, lm_weight=lw, bias=ctx,
                                                         bias_weight=bw)
    assert hyp.shape == (B, N, L) and score.dtype == torch.float64
    assert ("lm" in info) == with_lm and info["bias"].shape == (B, N)
    h_, l_, n_, s_ = (t.cpu().numpy() for t in (hyp, hyp_len, n_hyp, score))
    a_, c_, b_, f_ = (info[k].cpu().numpy() for k in ("att", "ctc", "bias", "finished"))
    m_ = info["lm"].cpu().numpy() if with_lm else np.zeros_like(a_)
    enc64, mask_c, z_c = enc.cpu().numpy(), mask.cpu().numpy(), z.cpu().numpy()
    decided = 0
    for b in range(B):
        T = int(mask_c[b].sum())
        got = [h_[b, k, :l_[b, k]].tolist() for k in range(n_[b])]
        fins = [bool(f_[b, k]) for k in range(n_[b])]
        for k in range(N):
            assert (h_[b, k, l_[b, k]:] == -1).all()
            if k >= n_[b]:
                assert l_[b, k] == 0 and s_[b, k] == a_[b, k] == c_[b, k] == b_[b, k] == NEG_INF
                continue
            want = ref.bias_fin(got[k]) if fins[k] else ref.bias(got[k])
            assert _bits(b_[b, k]) == _bits(want), (b, k, got[k])
            assert _bits(b_[b, k]) == _bits(ctx.bias_fin(got[k]) if fins[k] else ctx.bias(got[k]))
            if with_lm and fins[k]:
                assert m_[b, k] == ref_lm.seq_logprob(got[k]), (b, k)
            assert _bits(s_[b, k]) == _bits(br.bscore(w, lw, bw, a_[b, k], c_[b, k],
                                                      m_[b, k] if with_lm else 0.0, b_[b, k]))
        x = jr.log_softmax64(z_c[b, :T])
        logp64 = tj._memo(ar.model_logp(model64, enc64[b], mask_c[b]))
        logp32 = tj._memo(tj._existing_logp(model, enc[b], mask[b]))
        o = br.biased_search(logp64, x, ref, bw, N, K, L, w, ref_lm, lw)
        err = 0.0
        for slots in o.history:                   # A of every selected prefix on both models
            for s in slots:
                if s is not None:
                    a32 = 0.0
                    for j, v in enumerate(s.toks + ([EOS] if s.fin else [])):
                        a32 += float(logp32([s.toks[:j]])[0][v])
                    err = max(err, abs(s.A - a32))
        e = 4.0 * err + 1e-9 * max(1, T)
        decisive = o.margin >= 10 * e
        decided += decisive
        worst = max([abs(s_[b, k] - o.scores[k]) for k in range(min(n_[b], len(o.scores)))]
                    or [0.0])
        print(f"utt {b} (T={T}): e {e:.3e} oracle margin {o.margin:.3e} decisive {decisive} "
              f"device S diff {worst:.3e} finished {sum(fins)}/{n_[b]} "
              f"bias {b_[b, :n_[b]].tolist()}")
        if decisive:
            assert got == o.hyps and fins == o.finished, (b, got, o.hyps)
            for k in range(n_[b]):
                assert abs(s_[b, k] - o.scores[k]) <= e and abs(a_[b, k] - o.att[k]) <= e
                assert abs(c_[b, k] - o.ctc[k]) <= e
                assert _bits(b_[b, k]) == _bits(o.bias[k])
                if with_lm:
                    assert m_[b, k] == o.lm[k]
    if N == 1:
        assert decided >= 2, decided
    assert (b_[np.isfinite(b_)] > 0).any()          # the phrases are met


FORCED = [9, 17, 5, 30]


def _contains(toks, phrase):
    return any(toks[j:j + len(phrase)] == phrase for j in range(len(toks) - len(phrase) + 1))


@pytest.mark.parametrize("w", [0.0, 0.3])
def test_a_large_boost_forces_its_phrase_through_the_joint_search(gpu, w):
    from onebit_asr.attdec import joint_beam_search

    model, _ = tj._decoder_model(35, 64)
    enc, mask = tj._memory(0, 64, (61, 20, 12), gpu)
    with torch.no_grad():
        z = model.ctc_logits(enc)
    ctx = _ctx([FORCED], 50.0)
    hyp, hyp_len, n_hyp, _, info = joint_beam_search(model, enc, mask, z, 4, 10, w, 32, bias=ctx,
                                                     bias_weight=1.0)
    hyp0, len0, _, _, info0 = joint_beam_search(model, enc, mask, z, 4, 10, w, 32)
    assert "bias" not in info0
    for b in range(3):
        assert _contains(hyp[b, 0, :hyp_len[b, 0]].tolist(), FORCED)
        assert info["bias"][b, 0] >= 200.0
        assert not _contains(hyp0[b, 0, :len0[b, 0]].tolist(), FORCED)


def test_a_large_boost_forces_its_phrase_through_the_ctc_search(gpu):
    from onebit_asr.infer import ctc_beam_search_bias_device, ctc_beam_search_nbest_device

    model, _ = tj._decoder_model(35, 64)
    enc, mask = tj._memory(0, 64, (61, 20, 7), gpu)
    with torch.no_grad():
        z = model.ctc_logits(enc).float()
    lens = mask.sum(1)
    ctx = _ctx([FORCED], 50.0)
    hyp, hyp_len, n_hyp, info = ctc_beam_search_bias_device(z, lens, ctx, 1.0, beam_size=4,
                                                            blank_id=BLANK, top_k_per_t=None)
    p_hyp, p_len, _, _ = ctc_beam_search_nbest_device(z, lens, 4, None, BLANK, None)
    for b in range(3):
        assert _contains(hyp[b, 0, :hyp_len[b, 0]].tolist(), FORCED)
        assert info["bias"][b, 0] >= 200.0
        assert not _contains(p_hyp[b, 0, :p_len[b, 0]].tolist(), FORCED)


# ------------------------------------------------------------------------------------------
# 5. encode_and_decode: unchanged without a bias, graphed equals eager with one
# ------------------------------------------------------------------------------------------
def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        if isinstance(x, dict):
            assert x.keys() == y.keys(), (sorted(x), sorted(y))
            for k in x:
                assert x[k].dtype == y[k].dtype and _bytes(x[k]) == _bytes(y[k]), k
        else:
            assert x.dtype == y.dtype and _bytes(x) == _bytes(y)


@functools.lru_cache(maxsize=None)
def _full_model():
    from onebit_asr.conformer import ConformerASR
    from onebit_asr.data import CFG1, synthetic_batch

    torch.manual_seed(0)
    model = ConformerASR(80, 5004, **CFG1).to("cuda:0").eval()
    feat_lens, tok_lens = [349, 61], [12, 3]
    return model, [synthetic_batch(feat_lens, tok_lens, seed=s, device="cuda:0") for s in (0, 1)]


def _model_phrases(model, batches, decoder, kw):
    """Phrases cut from the n-best the decoder itself returns without a bias (so that the bias is
    met: their tokens are among its candidates) and a few others."""
    from onebit_asr.infer import encode_and_decode

    info = {}
    if decoder == "attention":
        encode_and_decode(model, batches[0], decoder=decoder, beam_size=4, info=info, **kw)
    else:       # the CTC n-best
        encode_and_decode(model, batches[0], decoder="rescore", beam_size=4, max_len=24, info=info)
    hyp, hyp_len = info["hyp"].cpu().numpy(), info["hyp_len"].cpu().numpy()
    phrases = [([4, 5, 6], 1.0), ([100, 200], 2.0)]
    for b in range(hyp.shape[0]):
        for k in range(4):
            toks = hyp[b, k, :hyp_len[b, k]].tolist()
            if len(toks) >= 2:
                phrases.append((toks[:3], 1.5))
                phrases.append((toks[-2:], 0.8))
    return phrases


DECODERS = [("greedy", {}), ("beam", {}), ("rescore", dict(max_len=24)),
            ("attention", dict(max_len=12)), ("attention", dict(max_len=12, joint_ctc_weight=0.3))]


@pytest.mark.parametrize("decoder,kw", DECODERS, ids=[d + ("-joint" if "joint_ctc_weight" in k
                                                           else "") for d, k in DECODERS])
def test_encode_and_decode_without_bias_weight_is_bitwise_unchanged(gpu, decoder, kw):
    from onebit_asr.infer import encode_and_decode
    from onebit_asr.quant import set_act_quant

    model, batches = _full_model()
    set_act_quant(model, None)
    ctx = _ctx(_model_phrases(model, batches, decoder, kw))
    runs = []
    for extra in ({}, dict(bias=ctx, bias_weight=0.0), dict(bias=None, bias_weight=0.0)):
        info = {}
        out, cnt, logits = encode_and_decode(model, batches[0], decoder=decoder, beam_size=4,
                                             info=info, **kw, **extra)
        runs.append((out, cnt, logits, info))
    _same(runs[0], runs[1])
    _same(runs[0], runs[2])
    assert "bias" not in runs[0][3]
    if decoder in ("greedy", "rescore"):
        with pytest.raises(ValueError, match="bias_weight"):
            encode_and_decode(model, batches[0], decoder=decoder, bias=ctx, bias_weight=0.5, **kw)
        return
    info = {}
    out, cnt, _ = encode_and_decode(model, batches[0], decoder=decoder, beam_size=4, info=info,
                                    bias=ctx, bias_weight=2.0, mbr_scale=1.0, timestamps=True,
                                    **kw)
    assert info["bias"].dtype == torch.float64 and info["bias"].shape == (2, 4)
    assert {"best_k", "mbr_risk", "map_k", "span", "align_score"} <= set(info)
    for b in range(2):
        k = int(info["best_k"][b])
        assert out[b, :cnt[b]].tolist() == info["hyp"][b, k, :info["hyp_len"][b, k]].tolist()
        for k in range(int(info["n_hyp"][b])):
            toks = info["hyp"][b, k, :info["hyp_len"][b, k]].tolist()
            closed = decoder == "beam" or bool(info["finished"][b, k])
            want = ctx.bias_fin(toks) if closed else ctx.bias(toks)
            assert _bits(info["bias"][b, k].item()) == _bits(want), (b, k)
    assert (info["bias"][torch.isfinite(info["bias"])] > 0).any()


GRAPHED = [("beam", {}, ("hyp", "hyp_len", "n_hyp", "ctc_scores", "lm", "bias", "total", "best_k")),
           ("attention", dict(max_len=12, joint_ctc_weight=0.3),
            ("hyp", "hyp_len", "n_hyp", "score", "finished", "trace_parent", "trace_token",
             "trace_score", "att", "ctc", "bias"))]


@pytest.mark.parametrize("decoder,kw,keys", GRAPHED, ids=[g[0] for g in GRAPHED])
def test_graphed_decoding_with_a_bias_equals_eager_bitwise(gpu, decoder, kw, keys):
    from onebit_asr.infer import GraphedInference, encode_and_decode
    from onebit_asr.quant import set_act_quant

    model, (b1, b2) = _full_model()
    set_act_quant(model, None)
    ctx = _ctx(_model_phrases(model, (b1, b2), decoder, kw))
    gi = GraphedInference(model, act_quant=None, decoder=decoder, beam_size=4, bias=ctx,
                          bias_weight=2.0, **kw)
    runs = []
    for b in (b1, b1, b2, b1):
        out, cnt, _ = gi.run(b)
        runs.append((out.clone(), cnt.clone(), {k: gi.info[k].clone() for k in keys}))
    assert gi.graph is not None
    set_act_quant(model, None)
    eager = []
    for b in (b1, b2):
        info = {}
        out, cnt, _ = encode_and_decode(model, b, decoder=decoder, beam_size=4, info=info,
                                        bias=ctx, bias_weight=2.0, **kw)
        eager.append((out, cnt, {k: info[k] for k in keys}))
    _same(runs[0], eager[0])
    _same(runs[1], runs[0])
    _same(runs[3], runs[0])
    _same(runs[2], eager[1])
    assert (eager[0][2]["bias"][torch.isfinite(eager[0][2]["bias"])] > 0).any()
