"""CPU: the n-gram LM of the shallow fusion (onebit_asr/ngram.py) -- ARPA parsing, the scoring
rule on hand-derived answers, the host table builder, and the kernels' probe routine on the host
(``ob_ngram_score_host``) against the dict oracle of tests/ngram_ref.py, bit for bit.

Known answers of tests/golden/ngram_tiny.arpa (a 3-gram model over the ids 5, 6, 7; values log10,
written x below; L(x) = float32(x * ln 10); the prefix is [<s>] + tokens):

  hit at order 3     P(6 | <s> 5)   = L(-0.125)                        entry (<s> 5 6)
  hit at order 2     P(5 | <s>)     = L(-0.25)                         entry (<s> 5)
  hit at order 3     P(</s> | 5 6)  = L(-0.0625)                       eos is scored as </s>
  full back-off      P(7 | 5 6)     = (L(-0.375) + L(-0.125)) + L(-1.25)
                                      (5 6 7) no; bo(5 6); (6 7) no; bo(6); unigram 7
  context no entry   P(6 | 7 5)     = L(-0.75)       (7 5 6) no; (7 5) is no entry: nothing added;
                                                     entry (5 6)
  context no entry   P(5 | 6 7)     = 0 + L(-0.5)    (6 7 5) no; (6 7) no entry; (7 5) no; bo(7) is
                                                     0 (none given); unigram 5
  unknown token      P(9 | <s> 5)   = (L(-0.5) + L(-0.25)) + L(-2.0)
                                      bo(<s> 5); bo(5); 9 has no unigram: <unk>'s value
  shorter than order P(6 | <s>)     = L(-0.5) + L(-1.5)                h = (<s>): bo(<s>); unigram 6
  sequence           lm([5, 6])     = (L(-0.25) + L(-0.125)) + L(-0.0625)
"""
import math

import numpy as np
import pytest

import ngram_ref as nr

LN10 = math.log(10.0)


def L(x):
    return float(np.float32(np.float64(x) * LN10))


@pytest.fixture(scope="module")
def tiny(golden_dir):
    from onebit_asr.ngram import NGramLM

    return NGramLM.from_arpa(golden_dir / "ngram_tiny.arpa")


def test_arpa_values_and_special_words(tiny, golden_dir):
    from onebit_asr.ngram import NGramLM

    assert tiny.order == 3 and tiny.n_entries == 11        # <unk> is no entry
    assert tiny.unk_logp == L(-2.0)
    assert tiny.score([], 5) == L(-0.25)                   # <s> is bos (1)
    assert tiny.score([5, 6], 2) == L(-0.0625)             # </s> is eos (2)
    text = (golden_dir / "ngram_tiny.arpa").read_text()
    same = NGramLM.from_arpa(text)                         # text in place of a path
    assert same.table.tobytes() == tiny.table.tobytes()
    assert NGramLM.from_arpa(text, unk_logp=-3.5).unk_logp == float(np.float32(-3.5))
    no_unk = text.replace("-2.0\t<unk>\n", "").replace("ngram 1=6", "ngram 1=5")
    assert NGramLM.from_arpa(no_unk).unk_logp == float(np.float32(math.log(1e-10)))


def test_arpa_vocab_mapping(tiny, golden_dir):
    from onebit_asr.ngram import NGramLM

    text = (golden_dir / "ngram_tiny.arpa").read_text()
    words = text.replace("\t5", "\tfive").replace(" 5", " five").replace("\t6", "\tsix") \
        .replace(" 6", " six").replace("\t7", "\tseven").replace(" 7", " seven")
    assert "five six" in words
    lm = NGramLM.from_arpa(words, vocab={"five": 5, "six": 6, "seven": 7})
    assert lm.table.tobytes() == tiny.table.tobytes()
    with pytest.raises(ValueError, match="line 10.*'five'"):
        NGramLM.from_arpa(words, vocab={"six": 6, "seven": 7})


@pytest.mark.parametrize("old,new,match", [
    ("-1.25\t7", "-1.25\t70000", "line 12.*70000"),                      # an id out of range
    ("-1.25\t7", "-1.25\t-7", "line 12"),
    ("-1.25\t7", "-1.25\tseven", "line 12.*decimal"),
    ("ngram 2=4", "ngram 2=5", "declares 5 2-grams.*holds 4"),           # a count mismatch
    ("ngram 3=2", "ngram 3=2\nngram 5=1", "line 5.*order 5"),            # order > 4
    ("-0.75\t5 6\t-0.375", "-0.75\t5 6 7 8\t-0.375", "line 16.*fields"),
    ("-0.75\t5 6\t-0.375", "x\t5 6", "line 16.*number"),
])
def test_arpa_malformed_input_names_the_line(golden_dir, old, new, match):
    from onebit_asr.ngram import NGramLM

    text = (golden_dir / "ngram_tiny.arpa").read_text()
    assert old in text
    with pytest.raises(ValueError, match=match):
        NGramLM.from_arpa(text.replace(old, new))


KNOWN = [
    ([5], 6, lambda: L(-0.125), "hit3"),
    ([], 5, lambda: L(-0.25), "hit2"),
    ([5, 6], 2, lambda: L(-0.0625), "hit3"),
    ([5, 6], 7, lambda: (L(-0.375) + L(-0.125)) + L(-1.25), "backoff_full"),
    ([7, 5], 6, lambda: L(-0.75), "ctx_missing"),
    ([6, 7], 5, lambda: 0.0 + L(-0.5), "ctx_missing"),
    ([5], 9, lambda: (L(-0.5) + L(-0.25)) + L(-2.0), "unk"),
    ([], 6, lambda: L(-0.5) + L(-1.5), "short"),
]


def _tiny_ref():
    e = {(1,): (L(-99), L(-0.5)), (2,): (L(-1.0), 0.0), (5,): (L(-0.5), L(-0.25)),
         (6,): (L(-1.5), L(-0.125)), (7,): (L(-1.25), 0.0), (1, 5): (L(-0.25), L(-0.5)),
         (5, 6): (L(-0.75), L(-0.375)), (6, 2): (L(-1.0), 0.0), (5, 7): (L(-0.625), 0.0),
         (1, 5, 6): (L(-0.125), 0.0), (5, 6, 2): (L(-0.0625), 0.0)}
    return nr.RefLM(e, 3, L(-2.0))


@pytest.mark.parametrize("toks,w,want,tag", KNOWN)
def test_known_answers(tiny, toks, w, want, tag):
    ref = _tiny_ref()
    got = tiny.score(toks, w)
    assert got == want(), (toks, w, got, want())
    val, tags = ref.score_detail(toks, w)
    assert val == got and tag in tags, (tags, val)         # the oracle agrees and names the case


def test_known_sequence_and_absent_candidate(tiny):
    assert tiny.seq_logprob([5, 6]) == (L(-0.25) + L(-0.125)) + L(-0.0625)
    assert tiny.seq_logprob([]) == _tiny_ref().seq_logprob([])
    assert tiny.score([5], -1) == -math.inf                # an absent candidate
    assert tiny.score_host(np.array([tiny.context([5])], np.uint64), np.array([6], np.int32),
                           vocab_size=6)[0] == (L(-0.5) + L(-0.25)) + L(-2.0)   # id >= V: no entry


def _mix(z):
    z = z.copy()
    z ^= z >> np.uint64(30)
    z *= np.uint64(0xbf58476d1ce4e5b9)
    z ^= z >> np.uint64(27)
    z *= np.uint64(0x94d049bb133111eb)
    z ^= z >> np.uint64(31)
    return z


def _check_layout(lm):
    """Power-of-two slots >= 2 x entries, every entry within max_probe <= 64 slots of its home with
    no empty slot on the way."""
    keys = lm.table[:, 0]
    assert lm.slots == keys.shape[0] and lm.slots & (lm.slots - 1) == 0
    assert lm.slots >= 2 * lm.n_entries and int((keys != 0).sum()) == lm.n_entries
    at = np.nonzero(keys)[0].astype(np.uint64)
    with np.errstate(over="ignore"):
        home = _mix(keys[at]) & np.uint64(lm.slots - 1)
    disp = (at - home) & np.uint64(lm.slots - 1)
    assert int(disp.max(initial=0)) + 1 == lm.max_probe <= 64
    far = np.argmax(disp) if len(disp) else 0
    for s in range(int(disp[far]) if len(disp) else 0):    # the longest run has no gap
        assert keys[(int(home[far]) + s) & (lm.slots - 1)] != 0


def test_table_is_deterministic_and_within_the_probe_bound():
    from onebit_asr.ngram import NGramLM

    entries, ids, n, vals = nr.random_lm(7, 4, 300, 20_000)
    a = NGramLM(entries, 4)
    order = list(entries)
    np.random.default_rng(0).shuffle(order)
    b = NGramLM({g: entries[g] for g in order}, 4)
    perm = np.random.default_rng(1).permutation(len(n))
    c = NGramLM.from_arrays(ids[perm], n[perm], vals[perm], 4)
    assert a.table.tobytes() == b.table.tobytes() == c.table.tobytes()
    assert (a.slots, a.max_probe) == (b.slots, b.max_probe) == (c.slots, c.max_probe)
    _check_layout(a)
    empty = NGramLM({}, 2)
    assert empty.slots == 8 and not empty.table.any() and empty.score([5], 6) == empty.unk_logp
    with pytest.raises(ValueError, match="distinct"):
        NGramLM.from_arrays(np.array([[5, 0, 0, 0], [5, 0, 0, 0]]), np.array([1, 1]),
                            np.zeros((2, 2), np.float32), 2)
    for bad in ({(5, 6, 7): (0.0, 0.0)}, {(70000,): (0.0, 0.0)}, {(-1,): (0.0, 0.0)}):
        with pytest.raises(ValueError):
            NGramLM(bad, 2)


def test_ids_0_and_65534_round_trip():
    from onebit_asr.ngram import NGramLM

    e = {(0,): (-1.5, -0.25), (65534,): (-2.5, -0.75), (0, 65534): (-0.5, -0.125),
         (65534, 0, 65534, 0): (-0.375, 0.0), (1, 0): (-3.0, 0.0)}
    lm, ref = NGramLM(e, 4), nr.RefLM(e, 4)
    for toks, w in [([], 0), ([], 65534), ([0], 65534), ([65534, 0, 65534], 0), ([0, 65534], 0),
                    ([65534], 65534), ([5, 0], 65534)]:
        assert lm.score(toks, w) == ref.score(toks, w), (toks, w)
    assert lm.score([65534, 0, 65534], 0) == -0.375 and lm.score([], 0) == -3.0


def test_host_scorer_equals_the_oracle_bit_for_bit_on_a_random_table():
    from onebit_asr.ngram import NGramLM

    V = 5004
    ref, ids, n, vals = nr.big_lm()
    lm = NGramLM.from_arrays(ids, n, vals, 4)
    assert lm.n_entries == len(ref.entries) >= 190_000
    _check_layout(lm)
    queries = nr.draw_queries(ref, V, 6000, 11)
    ctx = np.array([lm.context(t) for t, _ in queries], np.uint64)
    w = np.array([c for _, c in queries], np.int32)
    got, probes = lm.score_host(ctx, w, V, probes=True)
    cover = {}
    for (toks, c), g in zip(queries, got):
        want, tags = ref.score_detail(toks, c)
        assert g == want, (toks, c, g, want, tags)             # equal bits (or both -inf)
        for t in tags:
            cover[t] = cover.get(t, 0) + 1
    print(f"entries {lm.n_entries} slots {lm.slots} max_probe {lm.max_probe}; probes per query "
          f"mean {probes.mean():.2f} max {probes.max()}; outcomes {sorted(cover.items())}")
    for t in ("hit1", "hit2", "hit3", "hit4", "backoff_full", "ctx_missing", "unk", "short",
              "absent"):
        assert cover.get(t, 0) >= 20, (t, cover)
    assert 1 <= probes[w >= 0].min() and probes.max() <= 7 * lm.max_probe
