"""CPU: phrase-list contextual biasing (onebit_asr/bias.py, csrc/bias.hip, csrc/ob_bias.h): the rule
on hand-worked answers (the oracle of tests/bias_ref.py and the library's host walker both), the
builder's determinism and probe bound, the host walker against the oracle bit for bit, the oracle
searches at weight 0, the new symbols, their argument validation, the keyword pins and the
ValueErrors. The device side is tests/test_bias_gpu.py."""
import inspect

import numpy as np
import pytest

import bias_ref as br
from ctc_beam_lm_ref import lm_beam_search
from ctc_beam_ref import beam_search, ctc_like_logits
from ngram_ref import RefLM, random_lm

BLANK = 3
A, B, C, D, X = 10, 11, 12, 13, 20


def _bits(x):
    return np.asarray(x, np.float64).view(np.int64)


def _both(phrases, boost=1.0):
    from onebit_asr.bias import ContextBias

    return br.RefBias(phrases, boost), ContextBias(phrases, boost)


def _check(pair, tokens, bias, fin):
    """bias(y) and bias_fin(y) of the oracle and of the library's host walker."""
    ref, ctx = pair
    assert (ref.bias(tokens), ref.bias_fin(tokens)) == (bias, fin), tokens
    assert (ctx.bias(tokens), ctx.bias_fin(tokens)) == (bias, fin), tokens


def test_a_partial_match_is_taken_back():
    """Phrase "a b c", boost 2 per token. "a b" is two tokens into it: the running value counts
    val(2, 2) = 4, the closed value nothing. "a b x" leaves the phrase: (a, b) has no finished
    phrase to commit, its only proper suffix that is a node is the root, x starts nothing: 0. The
    whole phrase is a node without children: it commits val(3, 2) = 6 at once."""
    p = _both([[A, B, C]], 2.0)
    _check(p, [], 0.0, 0.0)
    _check(p, [A], 2.0, 0.0)
    _check(p, [A, B], 4.0, 0.0)
    _check(p, [A, B, X], 0.0, 0.0)
    _check(p, [A, B, C], 6.0, 6.0)
    _check(p, [A, B, C, A], 8.0, 6.0)
    _check(p, [X, A, B, C, X], 6.0, 6.0)


def test_a_phrase_and_its_extension_with_different_boosts():
    """ "a b" at 1 and "a b c" at 3: phi(a) = max(val(1, 1), val(1, 3)) = 3, commit(a b) = 2, phi(a b)
    = max(2, val(2, 3)) = 6, commit(a b c) = max(2, val(3, 3)) = 9. Leaving after "a b" keeps the 2
    and restarts at the root with the new token. With the boosts swapped the shorter phrase's 6
    outweighs the longer one's val(3, 1) = 3."""
    p = _both([([A, B], 1.0), ([A, B, C], 3.0)])
    _check(p, [A], 3.0, 0.0)
    _check(p, [A, B], 6.0, 2.0)
    _check(p, [A, B, C], 9.0, 9.0)
    _check(p, [A, B, X], 2.0, 2.0)
    _check(p, [A, B, A], 5.0, 2.0)          # the commit restarts at the root: (a) again
    _check(p, [A, B, A, B], 8.0, 4.0)
    q = _both([([A, B], 3.0), ([A, B, C], 1.0)])
    _check(q, [A, B], 6.0, 6.0)
    _check(q, [A, B, C], 6.0, 6.0)


def test_the_failure_link_recovers_an_overlapping_start():
    """Phrase "a b a c" on "a b a b a c": at (a, b, a) the token b has no edge and nothing to commit;
    the longest proper suffix that is a node is (a), which has the edge b: (a, b), no restart from
    the root. Two tokens later the phrase completes: val(4, 1) = 4."""
    ref, ctx = p = _both([[A, B, A, C]])
    tags = set()
    assert ref.walk([A, B, A, B], tags)[0] == (A, B) and "edge_after_fail" in tags
    _check(p, [A, B, A], 3.0, 0.0)
    _check(p, [A, B, A, B], 2.0, 0.0)
    _check(p, [A, B, A, B, A, C], 4.0, 4.0)
    assert ctx.walk([A, B, A, B])[0] == br.node_numbers(ref)[(A, B)] == 2


def test_a_commit_on_the_fail_path():
    """ "a b c d" at 1 and "b c" at 2 on "a b c x": (a, b, c) has no edge x and no finished phrase;
    its fail link is (b, c), which has no edge x either but is a finished phrase: val(2, 2) = 4 is
    kept and matching restarts at the root."""
    ref, _ = p = _both([([A, B, C, D], 1.0), ([B, C], 2.0)])
    tags = set()
    ref.walk([A, B, C, X], tags)
    assert "commit_on_fail_path" in tags
    _check(p, [A, B, C], 3.0, 0.0)
    _check(p, [A, B, C, X], 4.0, 4.0)
    _check(p, [A, B, C, D], 4.0, 4.0)
    _check(p, [B, C], 4.0, 4.0)


def test_a_single_token_phrase():
    p = _both([[A]], 2.5)
    _check(p, [A], 2.5, 2.5)
    _check(p, [A, A], 5.0, 5.0)
    _check(p, [X, A, X], 2.5, 2.5)


def test_a_duplicate_phrase_keeps_the_larger_boost():
    from onebit_asr.bias import ContextBias

    p = _both([([A, B], 1.0), ([A, B], 4.0), ([A, B], 2.0)])
    _check(p, [A, B], 8.0, 8.0)
    one = ContextBias([([A, B], 4.0)])
    assert p[1].nodes.tobytes() == one.nodes.tobytes()
    assert p[1].edges.tobytes() == one.edges.tobytes()


def _random_phrases(seed, V, count, max_len=5):
    rng = np.random.default_rng(seed)
    boosts = (0.5, 1.0, 1.7, 2.3, 0.3)
    out = []
    for _ in range(count):
        n = int(rng.integers(1, max_len + 1))
        out.append(([int(t) for t in rng.integers(4, V, size=n)],
                    boosts[int(rng.integers(len(boosts)))]))
    return out


def test_builder_is_deterministic_and_bounded():
    from onebit_asr.bias import ContextBias

    for V, count in ((7, 30), (40, 60), (5004, 1000)):
        phrases = _random_phrases(11 + V, V, count)
        if V == 40:
            phrases.append((list(range(4, 20)), 0.7))           # the longest phrase allowed
        ctx = ContextBias(phrases)
        ref = br.RefBias(phrases)
        assert ctx.n_nodes == len(ref.nodes)
        assert 1 <= ctx.max_probe <= 64
        assert ctx.slots & (ctx.slots - 1) == 0 and ctx.slots >= 2 * (ctx.n_nodes - 1)
        rng = np.random.default_rng(V)
        for _ in range(3):
            perm = [phrases[i] for i in rng.permutation(len(phrases))]
            other = ContextBias(perm)
            assert other.nodes.tobytes() == ctx.nodes.tobytes()
            assert other.edges.tobytes() == ctx.edges.tobytes()
            assert (other.slots, other.max_probe) == (ctx.slots, ctx.max_probe)
        # the records are the definitions', node by node, in the contract's numbering
        num = br.node_numbers(ref)
        rec = ctx.nodes.view(np.int32).reshape(-1, 4)
        flt = ctx.nodes.view(np.float32).reshape(-1, 4)
        for p, k in list(num.items())[:400]:
            assert rec[k, 0] == num[ref.fail(p)] and (rec[k, 1] & 1) == int(ref.has_children(p))
            assert flt[k, 2] == np.float32(ref.phi(p)) and flt[k, 3] == np.float32(ref.commit(p))


@pytest.mark.parametrize("V", [7, 40, 5004])
def test_host_walker_equals_the_oracle_bit_for_bit(V):
    from onebit_asr.bias import ContextBias

    phrases = _random_phrases(50 + V, V, 6 if V == 7 else 80)
    longer = [ids for ids, _ in phrases if len(ids) >= 3]
    phrases += [(ids[:2], 1.9) for ids in longer[:4]]           # finished phrases with children
    four = [ids for ids in longer[4:] if len(ids) >= 4] or [[4, 5, 6, 4, 5]]
    phrases += [(ids, 0.4) for ids in four[:1]]
    phrases += [(ids[1:3], 0.9) for ids in four[:4]]            # and on the fail path
    if V == 40:
        phrases.append((list(range(4, 20)), 0.7))
        phrases.append((list(range(5, 12)), 1.3))
    ctx, ref = ContextBias(phrases), br.RefBias(phrases)
    num = br.node_numbers(ref)
    rng = np.random.default_rng(V)
    Q, T = 2000, 24
    toks = np.full((Q, T), -1, np.int32)
    lens = np.zeros(Q, np.int32)
    for q in range(Q):
        seq = []
        while len(seq) < T and rng.random() < 0.93:
            kind = rng.integers(4)
            if kind == 0:
                seq.append(int(rng.integers(4, V)))
            else:                                               # a phrase, whole or cut short
                ids = phrases[int(rng.integers(len(phrases)))][0]
                cut = len(ids) if kind == 1 else int(rng.integers(1, len(ids) + 1))
                seq += ids[:cut]
        seq = seq[:T]
        toks[q, :len(seq)] = seq
        lens[q] = len(seq)
    state, kept, bias, fin = ctx.walk_host(toks, lens)
    tags = set()
    for q in range(Q):
        s, k, b, f = ref.walk(toks[q, :lens[q]].tolist(), tags)
        assert state[q] == num[s], q
        assert _bits(kept[q]) == _bits(k) and _bits(bias[q]) == _bits(b), q
        assert _bits(fin[q]) == _bits(f), q
    want = {"edge", "edge_after_fail", "commit", "commit_on_fail_path", "restart_hit",
            "restart_miss", "root_miss", "leaf"}
    if V == 7:      # three usable ids: every one starts a phrase, nothing misses at the root
        want -= {"commit_on_fail_path", "restart_miss", "root_miss"}
    assert want <= tags, want - tags
    assert (bias > fin).any() and (kept > 0).any() and lens.min() == 0


def test_oracle_search_at_weight_zero_is_the_searches_of_today():
    V, T = 12, 24
    logits = ctc_like_logits(77, 2, T, V, BLANK)
    entries, _, _, _ = random_lm(5, 3, V, 40 * V)
    lm = RefLM(entries, 3)
    ref = br.RefBias(_random_phrases(3, V, 10, 3))
    for b in range(2):
        x = logits[b]
        with_lm = lm_beam_search(x, lm, 0.3, 0.5, 6, BLANK, 20)
        got = br.biased_beam_search(x, ref, 0.0, lm, 0.3, 0.5, 6, BLANK, 20)
        assert got.final_beam == with_lm.final_beam and got.merges == with_lm.merges
        assert [e[1:3] + e[4:] for e in got.beam] == [e[1:] for e in with_lm.beam]
        assert got.margin == with_lm.margin and got.gap == with_lm.gap
        plain = beam_search(x, 6, BLANK, 20)
        none = br.biased_beam_search(x, ref, 0.0, None, 0.0, 0.0, 6, BLANK, 20)
        assert none.final_beam == plain.final_beam and none.beam[0][1] == plain.score
        assert all(e[2] == 0.0 for e in none.beam)
        # and the bias term changes the search
        on = br.biased_beam_search(x, br.RefBias([plain.final_beam[2][:3]], 5.0), 1.0, None, 0.0,
                                   0.0, 6, BLANK, 20)
        assert on.beam[0][3] > 0 and on.beam[0][4] == on.beam[0][1] + 1.0 * on.beam[0][3]


# ------------------------------------------------------------------------------------------
# the surface
# ------------------------------------------------------------------------------------------
NEW = {"ob_bias_supported": 3, "ob_bias_sizes": 4, "ob_bias_build": 11, "ob_bias_walk_host": 13,
       "ob_bias_step": 20, "ob_bias_seq_score": 11, "ob_attdec_biased_step": 33,
       "ob_ctc_beam_search_bias_workspace": 7, "ob_ctc_beam_search_bias": 34}


def test_symbols_are_exported_with_signatures():
    import ctypes

    import onebit_asr
    from onebit_asr import _lib, attdec, bias, infer

    lib = _lib.load()
    for name, nargs in NEW.items():
        res, args = _lib.SIGNATURES[name]
        assert len(args) == nargs and getattr(lib, name).argtypes == args, name
    assert _lib.SIGNATURES["ob_ctc_beam_search_bias_workspace"][0] is ctypes.c_size_t
    assert lib.ob_abi_version() == 4                                # entries were only added
    assert _lib.SIGNATURES["ob_attdec_biased_step"][1][:7] == \
        _lib.SIGNATURES["ob_attdec_fused_step"][1][:7]
    assert bias.__all__ == ["ContextBias", "bias_step", "bias_seq_score", "MAX_PHRASE_LEN",
                            "MAX_ID"]
    for name in ("ContextBias", "bias_step", "bias_seq_score"):
        assert getattr(onebit_asr, name) is getattr(bias, name)
    assert onebit_asr.ctc_beam_search_bias_device is infer.ctc_beam_search_bias_device
    assert "ctc_beam_search_bias_device" in infer.__all__
    p = inspect.signature(infer.ctc_beam_search_bias_device).parameters
    assert list(p) == ["logits", "lens", "bias", "bias_weight", "lm", "lm_weight", "ins_bonus",
                       "beam_size", "nbest", "blank_id", "top_k_per_t"]
    assert [p[k].default for k in list(p)[4:]] == [None, 0.0, 0.0, 10, None, 3, 20]
    # the LM search keeps its parameter list
    assert list(inspect.signature(infer.ctc_beam_search_lm_device).parameters) == [
        "logits", "lens", "lm", "lm_weight", "ins_bonus", "beam_size", "nbest", "blank_id",
        "top_k_per_t"]
    j = inspect.signature(attdec.joint_beam_search).parameters
    assert list(j)[-4:] == ["lm", "lm_weight", "bias", "bias_weight"]
    assert (j["bias"].default, j["bias_weight"].default) == (None, 0.0)
    # the mode tuple knows no bias
    assert tuple(attdec._search_mode(4, None, True, 0.3, None, 0.0)) == (
        "ob_attdec_joint_step", 8, True, False, ("att", "ctc"))
    assert len(attdec._SearchMode._fields) == 5
    assert "score_bias" in vars(attdec._BeamSearch)
    assert lib.ob_bias_supported(5004, 20, 100) == 1 and lib.ob_bias_supported(65535, 32, 1) == 1
    assert lib.ob_bias_supported(65536, 20, 100) == 0 and lib.ob_bias_supported(40, 33, 100) == 0
    assert lib.ob_bias_supported(40, 20, 0) == 0


def test_context_bias_rejects_bad_phrases():
    from onebit_asr import _lib
    from onebit_asr.bias import ContextBias

    for bad in ([[]], [list(range(4, 21))], [[-1]], [[65535]], [([4], 0.0)], [([4], -1.0)],
                [([4], float("nan"))], [([4], float("inf"))], [([4], 1e39)]):
        with pytest.raises(ValueError):
            ContextBias(bad)
    assert ContextBias([]).n_nodes == 1 and ContextBias([]).bias([4, 5]) == 0.0
    got = ContextBias.from_text(["ab", ("c", 3.0)], lambda s: [ord(ch) for ch in s], 2.0)
    assert got.bias_fin([97, 98]) == 4.0 and got.bias_fin([99]) == 3.0
    # the C entry itself
    lib = _lib.load()
    import ctypes
    n_nodes, slots, probe = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int32(0)
    outs = (ctypes.addressof(n_nodes), ctypes.addressof(slots), ctypes.addressof(probe))
    nodes, edges = np.zeros((8, 4), np.int32), np.zeros((8, 2), np.uint64)
    bufs = (nodes.ctypes.data, nodes.nbytes, edges.ctypes.data, edges.nbytes)

    def build(toks, lens, boosts):
        t, n, b = np.asarray(toks, np.int32), np.asarray(lens, np.int32), \
            np.asarray(boosts, np.float32)
        return lib.ob_bias_build(t.ctypes.data, n.ctypes.data, b.ctypes.data, len(lens), *bufs,
                                 *outs)
    NULL, SHAPE, WORKSPACE, ALIGN = -1, -2, -4, -5
    assert build([4, 5], [2], [1.0]) == 0 and (n_nodes.value, slots.value) == (3, 8)
    for toks, lens, boosts in (([4], [0], [1.0]), (list(range(17)), [17], [1.0]), ([-1], [1], [1.0]),
                               ([65535], [1], [1.0]), ([4], [1], [0.0]), ([4], [1], [-2.0]),
                               ([4], [1], [np.nan]), ([4], [1], [np.inf])):
        assert build(toks, lens, boosts) == SHAPE, (toks, lens, boosts)
    assert build(list(range(4, 14)), [10], [1.0]) == WORKSPACE and n_nodes.value == 11
    assert slots.value == 32
    t = np.asarray([4], np.int32)
    assert lib.ob_bias_build(None, t.ctypes.data, t.ctypes.data, 1, *bufs, *outs) == NULL
    assert lib.ob_bias_build(t.ctypes.data, t.ctypes.data, t.ctypes.data, 1, *bufs, None,
                             outs[1], outs[2]) == NULL
    assert lib.ob_bias_build(t.ctypes.data, t.ctypes.data, t.ctypes.data, 1, bufs[0] + 8, 64,
                             bufs[2], bufs[3], *outs) == ALIGN
    mx, mn = ctypes.c_int64(0), ctypes.c_int64(0)
    assert lib.ob_bias_sizes(3, 10, ctypes.addressof(mx), ctypes.addressof(mn)) == 0
    assert (mx.value, mn.value) == (11, 32)
    assert lib.ob_bias_sizes(3, 2, ctypes.addressof(mx), ctypes.addressof(mn)) == SHAPE
    assert lib.ob_bias_sizes(3, 49, ctypes.addressof(mx), ctypes.addressof(mn)) == SHAPE
    assert lib.ob_bias_sizes(3, 10, None, ctypes.addressof(mn)) == NULL


def test_argument_validation_without_gpu():
    """Every check below fails before any HIP call, so it is safe with no device."""
    from onebit_asr import _lib

    lib = _lib.load()
    ws = lib.ob_ctc_beam_search_bias_workspace
    assert ws(32, 249, 5004, 10, 20, 4, 3000) == ws(32, 249, 5004, 10, 20, 0, 3000) == \
        lib.ob_ctc_beam_search_nbest_workspace(32, 249, 5004, 10, 20) > 0
    assert ws(2, 16, 5004, 10, 20, 5, 10) == 0 and ws(2, 16, 65536, 10, 20, 0, 10) == 0
    assert ws(2, 16, 5004, 10, 20, 0, 0) == 0 and ws(2, 16, 5004, 33, 20, 0, 10) == 0
    f = 0x1000
    NULL, SHAPE, WORKSPACE, ALIGN = -1, -2, -4, -5
    nan, inf = float("nan"), float("inf")

    def search(**kw):
        a = dict(logits=f, lens=f, B=2, T=16, V=40, blank=3, beam=10, top_k=20, nbest=10, table=f,
                 slots=64, max_probe=4, order=3, unk=-23.0, bos=1, eos=2, lw=0.5, bonus=0.0,
                 nodes=f, n_nodes=9, edges=f, bslots=16, bprobe=2, bw=1.0, ws=f, ws_bytes=1 << 30,
                 hyp=f, hyp_len=f, n_hyp=f, ctc=f, lm=f, bias=f, total=f)
        a.update(kw)
        return lib.ob_ctc_beam_search_bias(*a.values(), None)
    for kw in (dict(order=5), dict(V=65536), dict(beam=33, nbest=33), dict(top_k=65),
               dict(nbest=11), dict(blank=40), dict(bos=40), dict(slots=48), dict(max_probe=65),
               dict(lw=-0.5), dict(lw=nan), dict(bonus=inf), dict(unk=-inf), dict(n_nodes=0),
               dict(bslots=24), dict(bslots=4), dict(bprobe=0), dict(bprobe=65), dict(bw=-1.0),
               dict(bw=nan), dict(bw=inf), dict(table=None, lw=0.5), dict(table=None, lw=0.0, bonus=nan)):
        assert search(**kw) == SHAPE, kw
    for name in ("logits", "lens", "nodes", "edges", "ws", "hyp", "hyp_len", "n_hyp", "ctc", "lm",
                 "bias", "total"):
        assert search(**{name: None}) == NULL, name
        assert search(table=None, lw=0.0, **{name: None}) == NULL, name
    for name in ("lens", "ws", "ctc", "lm", "bias", "total"):                       # 8-byte
        assert search(**{name: 0x3004}) == ALIGN, name
    for name in ("logits", "hyp", "hyp_len", "n_hyp"):
        assert search(**{name: 0x3002}) == ALIGN, name
    for name in ("table", "nodes", "edges"):                                        # 16-byte
        assert search(**{name: 0x3008}) == ALIGN, name
    assert search(ws_bytes=8) == WORKSPACE
    assert search(table=None, lw=0.0, ws_bytes=8) == WORKSPACE      # the form without an LM
    assert search(B=0, logits=None, lens=None, hyp=None, bias=None) == 0            # no launch

    def step(**kw):
        a = dict(nodes=f, n_nodes=9, edges=f, slots=16, probe=2, topi=f, tok=f, len=f, link=f,
                 skip=f, B=2, N=4, K=8, eos=2, st_in=f, st_out=0x2000, kept_in=f, kept_out=0x2000,
                 bsc=f)
        a.update(kw)
        return lib.ob_bias_step(*a.values(), None)
    for kw in (dict(n_nodes=0), dict(slots=12), dict(probe=65), dict(K=33), dict(K=0), dict(N=0),
               dict(N=33), dict(B=-1), dict(eos=-1), dict(st_out=f), dict(kept_out=f)):
        assert step(**kw) == SHAPE, kw
    for name in ("nodes", "edges", "topi", "tok", "len", "link", "skip", "st_in", "st_out",
                 "kept_in", "kept_out", "bsc"):
        assert step(**{name: None}) == NULL, name
    for name in ("tok", "kept_in", "kept_out", "bsc"):
        assert step(**{name: 0x3004}) == ALIGN, name
    for name in ("topi", "len", "link", "st_in", "st_out"):
        assert step(**{name: 0x3002}) == ALIGN, name
    assert step(nodes=0x3008) == ALIGN and step(edges=0x3008) == ALIGN
    assert step(B=0, topi=None, bsc=None) == 0

    def seq(**kw):
        a = dict(nodes=f, n_nodes=9, edges=f, slots=16, probe=2, hyp=f, hyp_len=f, R=3, T=8, out=f)
        a.update(kw)
        return lib.ob_bias_seq_score(*a.values(), None)
    assert seq(R=-1) == SHAPE and seq(T=-1) == SHAPE and seq(slots=0) == SHAPE
    for name in ("nodes", "edges", "hyp", "hyp_len", "out"):
        assert seq(**{name: None}) == NULL, name
    assert seq(out=0x3004) == ALIGN and seq(hyp=0x3002) == ALIGN and seq(nodes=0x3008) == ALIGN
    assert seq(R=0, hyp=None) == 0

    def biased(**kw):
        a = dict(lse=f, topv=f, topi=f, cpsi=f, w=0.25, lmsc=f, lw=0.5, bsc=f, bw=1.0, B=2, N=4,
                 K=8, L=6, t=0, eos=2, pad=0, norm=f, anc_in=f, anc_out=0x2000, score=f, att=f,
                 ctc=f, lm=f, bias=f, len=f, fin=f, tok=f, skip=f, link=f, trp=f, trt=f, trs=f)
        a.update(kw)
        return lib.ob_attdec_biased_step(*a.values(), None)
    for kw in (dict(bw=-1.0), dict(bw=nan), dict(bw=inf), dict(lw=nan), dict(w=1.5), dict(K=3),
               dict(K=33), dict(t=6), dict(lmsc=None, lw=0.5), dict(anc_out=f)):
        assert biased(**kw) == SHAPE, kw
    for name in ("lse", "topv", "topi", "cpsi", "bsc", "norm", "anc_in", "anc_out", "score", "att",
                 "ctc", "lm", "bias", "len", "fin", "tok", "skip", "link", "trp", "trt", "trs"):
        assert biased(**{name: None}) == NULL, name
    # without an LM: lmsc and lm may both be null, and cpsi too when w == 0
    assert biased(lmsc=None, lm=None, lw=0.0, bsc=None) == NULL
    assert biased(lmsc=None, lm=None, lw=0.0, w=0.0, cpsi=None, bias=None) == NULL
    for name in ("lse", "bsc", "bias", "lm", "score", "trs"):
        assert biased(**{name: 0x3004}) == ALIGN, name
    assert biased(B=0, lse=None, bsc=None, bias=None) == 0


def test_bias_keywords_are_pinned():
    from onebit_asr.infer import GraphedInference, encode_and_decode

    for fn in (encode_and_decode, GraphedInference.__init__):
        p = inspect.signature(fn).parameters
        names = list(p)
        assert names[-4:] == ["lm_fusion", "ins_bonus", "joint_ctc_weight", "ctc_cand"]
        assert names.index("timestamps") + 1 == names.index("mbr_scale")
        assert names.index("mbr_scale") + 1 == names.index("bias")
        assert names.index("bias") + 1 == names.index("bias_weight")
        assert names.index("lm_weight") + 1 == names.index("lm_fusion")
        assert (p["bias"].default, p["bias_weight"].default) == (None, 0.0)
        assert p["bias"].kind is p["bias_weight"].kind is inspect.Parameter.KEYWORD_ONLY


def test_bias_value_errors():
    import torch

    from onebit_asr.attdec import joint_beam_search
    from onebit_asr.bias import ContextBias
    from onebit_asr.infer import GraphedInference, ctc_beam_search_bias_device, encode_and_decode

    class FakeLM:            # the checks run ahead of the forward: nothing of the LM is touched
        bos, eos, order = 1, 2, 3

    lm, ctx = FakeLM(), ContextBias([[4, 5]])

    def both(match, **kw):
        with pytest.raises(ValueError, match=match):
            encode_and_decode(None, {}, **kw)
        with pytest.raises(ValueError, match=match):
            GraphedInference(torch.nn.Identity(), act_quant=None, **kw)
    for dec in ("greedy", "rescore"):
        both("bias_weight", decoder=dec, bias=ctx, bias_weight=1.0)
    for dec in ("greedy", "beam", "rescore", "attention"):
        both("bias_weight", decoder=dec, bias_weight=1.0)                        # no bias object
        for w in (-0.5, float("nan"), float("inf")):
            both("bias_weight", decoder=dec, bias=ctx, bias_weight=w)
    both("first_pass", decoder="beam", bias=ctx, bias_weight=1.0, lm=lm, lm_weight=0.5)
    gi = GraphedInference(torch.nn.Identity(), act_quant=None, decoder="beam", bias=ctx,
                          bias_weight=1.5, lm=lm, lm_weight=0.5, lm_fusion="first_pass")
    assert (gi.bias, gi.bias_weight, gi.lm_fusion) == (ctx, 1.5, "first_pass")
    # weight 0 is no bias at all: every decoder takes it
    for dec in ("greedy", "beam", "rescore", "attention"):
        GraphedInference(torch.nn.Identity(), act_quant=None, decoder=dec, bias=ctx)
    z = torch.zeros(2, 9, 40)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ctc_beam_search_bias_device(z, torch.tensor([9, 3]), ctx, 1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        joint_beam_search(None, z, z[:, :, 0], z, bias=ctx, bias_weight=1.0)
