"""CPU: the edit-distance oracle (tests/edit_ref.py) against ``metrics.levenshtein_distance``, its
numpy form, its identities and the hand-derived cases; the exact-tie rule of the MBR pick; the
argument validation of every new C entry (before any HIP call); the Python surface."""
import inspect
import json
import math
import random

import pytest

from edit_ref import edit_distance_np, edit_ops, mbr, pairwise

OK, NULL, SHAPE, WS, ALIGN = 0, -1, -2, -4, -5


@pytest.fixture(scope="module")
def kat(golden_dir):
    return json.loads((golden_dir / "edit_kat.json").read_text())


def test_tuple_dp_agrees_with_levenshtein_and_numpy_and_keeps_its_identities():
    from onebit_asr.metrics import levenshtein_distance

    rng = random.Random(5)
    for alphabet in (2, 4, 50):
        for _ in range(150):
            a = [rng.randrange(alphabet) for _ in range(rng.randint(0, 20))]
            b = [rng.randrange(alphabet) for _ in range(rng.randint(0, 20))]
            d, sub, ins, dele = edit_ops(a, b)
            assert d == levenshtein_distance(a, b) == edit_distance_np(a, b), (a, b)
            assert d == sub + ins + dele, (a, b)
            assert len(b) - len(a) == ins - dele, (a, b)
            assert min(sub, ins, dele) >= 0
    assert edit_ops([], []) == (0, 0, 0, 0)
    assert edit_ops([7] * 5, [7] * 5) == (0, 0, 0, 0)


def test_hand_derived_cases(kat):
    assert len(kat["edit"]) >= 5
    for case in kat["edit"]:
        assert list(edit_ops(case["a"], case["b"])) == case["want"], case
        assert edit_distance_np([ord(c) for c in case["a"]],
                                [ord(c) for c in case["b"]]) == case["want"][0], case


def test_mbr_exact_ties_go_to_the_smaller_k(kat):
    sizes = set()
    for case in kat["mbr"]:
        n_slots = len(case["entries"])
        sizes.add(n_slots)
        assert case["scale"] == 0.0
        dpair = pairwise(case["entries"], case["n"], n_slots)
        assert dpair == case["dpair"], case
        best, risk, post = mbr(dpair, case["scores"], case["n"], case["scale"])
        assert post == case["post"], case
        assert risk == [float(r) for r in case["risk"]], case  # equal bits, not close
        assert best == case["best_k"], case
        live = risk[:case["n"]]
        assert live.count(min(live)) >= 2 and live.index(min(live)) == best  # a real tie
    assert sizes == {2, 4}


def test_mbr_oracle_rules():
    dpair = [[0, 2, -1], [2, 0, -1], [-1, -1, -1]]
    ninf = -math.inf
    # no live entry, and a largest live score of -inf: entry 0, every risk +inf, every post 0
    assert mbr(dpair, [0.0, 0.0, 0.0], 0, 1.0) == (0, [math.inf] * 3, [0.0] * 3)
    assert mbr(dpair, [ninf, ninf, 0.0], 2, 1.0) == (0, [math.inf] * 3, [0.0] * 3)
    # a large scale is the MAP entry; an entry at -inf weighs nothing at any scale
    best, risk, post = mbr(dpair, [-3.0, -1.0, 0.0], 2, 1e4)
    assert best == 1 and post[:2] == [0.0, 1.0] and risk == [2.0, 0.0, math.inf]
    best, risk, post = mbr(dpair, [ninf, -1.0, 0.0], 2, 0.0)
    assert best == 1 and post == [0.0, 1.0, 0.0] and risk == [2.0, 0.0, math.inf]


def test_edit_distance_validation_without_gpu():
    """Every check below fails before any HIP call, so it is safe with no device."""
    from onebit_asr import _lib

    lib = _lib.load()
    f = 0x3000  # never dereferenced
    assert lib.ob_edit_supported(0, 0) == 1 and lib.ob_edit_supported(4096, 4096) == 1
    assert lib.ob_edit_supported(4097, 5) == 0 and lib.ob_edit_supported(5, 4097) == 0
    assert lib.ob_edit_supported(-1, 5) == 0 and lib.ob_edit_supported(5, -1) == 0
    ws = lib.ob_edit_distance_workspace
    assert ws(4, 7, 4097) == 0 and ws(4, 4097, 7) == 0 and ws(-1, 7, 5) == 0
    assert ws(1 << 31, 7, 5) == 0 and ws((1 << 31) - 1, 7, 5) > 0
    need = ws(6, 200, 130)
    assert need >= 130 * 8 and need % 8 == 0
    assert ws(1 << 20, 200, 130) == ws(1 << 24, 200, 130)  # bounded by the waves in flight
    print(f"workspace: 6 pairs of 200 x 130: {need} bytes; any number of pairs at 4096 x 4096: "
          f"{ws(1 << 24, 4096, 4096)} bytes")

    # a, a_len, b, b_len, P, La, Lb, ws, ws_bytes, dist, ops
    def call(**kw):
        args = dict(a=f, a_len=f, b=f, b_len=f, P=6, La=200, Lb=130, ws=f, ws_bytes=need - 1,
                    dist=f, ops=f)
        args.update(kw)
        return lib.ob_edit_distance(*args.values(), None)
    assert call() == WS                                   # one byte short, everything else valid
    assert call(ops=None) == WS                           # ops may be null
    assert call(La=4097) == SHAPE and call(Lb=4097) == SHAPE and call(La=-1) == SHAPE
    assert call(Lb=-1) == SHAPE and call(P=-1) == SHAPE and call(P=1 << 31) == SHAPE
    for name in ("a", "a_len", "b", "b_len", "ws", "dist"):
        assert call(**{name: None}) == NULL, name
    for name in ("a", "a_len", "b", "b_len", "dist", "ops"):
        assert call(**{name: 0x3002}) == ALIGN, name
    assert call(ws=0x3004) == ALIGN                       # 8-byte
    # a zero width needs no array
    assert call(La=0, a=None, ws_bytes=ws(6, 0, 130) - 1) == WS
    assert call(Lb=0, b=None, ws_bytes=ws(6, 200, 0) - 1) == WS
    assert call(P=0, **{k: None for k in ("a", "a_len", "b", "b_len", "ws", "dist", "ops")}) == OK


def test_nbest_edit_distance_validation_without_gpu():
    from onebit_asr import _lib

    lib = _lib.load()
    f = 0x3000
    ws = lib.ob_nbest_edit_distance_workspace
    need = ws(4, 5, 40, 30)
    assert need > 0 and ws(4, 0, 40, 30) == 0 and ws(4, 33, 40, 30) == 0
    assert ws(4, 5, 4097, 30) == 0 and ws(4, 5, 40, 4097) == 0 and ws(-1, 5, 40, 30) == 0
    assert ws(1 << 31, 32, 40, 30) == 0                   # B * N * (N + 3) / 2 >= 2^31
    assert ws(4, 32, 4096, 4096) > 0

    # hyp, hyp_len, n_hyp, ref, ref_len, B, N, T, S, ws, ws_bytes, dref, ops_ref, dpair
    def call(**kw):
        args = dict(hyp=f, hyp_len=f, n_hyp=f, ref=f, ref_len=f, B=4, N=5, T=40, S=30, ws=f,
                    ws_bytes=need - 1, dref=f, ops_ref=f, dpair=f)
        args.update(kw)
        return lib.ob_nbest_edit_distance(*args.values(), None)
    assert call() == WS
    assert call(N=0) == SHAPE and call(N=33) == SHAPE and call(T=4097) == SHAPE
    assert call(S=4097) == SHAPE and call(T=-1) == SHAPE and call(B=-1) == SHAPE
    for name in ("hyp", "hyp_len", "n_hyp", "ref", "ref_len", "ws"):
        assert call(**{name: None}) == NULL, name
    assert call(dref=None, ops_ref=None, dpair=None) == NULL          # nothing to compute
    # each output may be absent; without dref and ops_ref the reference is not needed
    assert call(dpair=None) == WS and call(ops_ref=None) == WS and call(dref=None) == WS
    assert call(dref=None, ops_ref=None, ref=None, ref_len=None) == WS
    assert call(dpair=None, ref=None) == NULL
    for name in ("hyp", "hyp_len", "n_hyp", "ref", "ref_len", "dref", "ops_ref", "dpair"):
        assert call(**{name: 0x3002}) == ALIGN, name
    assert call(ws=0x3004) == ALIGN
    assert call(T=0, hyp=None, ws_bytes=ws(4, 5, 0, 30) - 1) == WS
    assert call(S=0, ref=None, ws_bytes=ws(4, 5, 40, 0) - 1) == WS
    everything = ("hyp", "hyp_len", "n_hyp", "ref", "ref_len", "ws", "dref", "ops_ref", "dpair")
    assert call(B=0, **{k: None for k in everything}) == OK


def test_mbr_select_validation_without_gpu():
    from onebit_asr import _lib

    lib = _lib.load()
    f = 0x3000

    # dpair, hyp, hyp_len, n_hyp, score, scale, B, N, T, out, out_len, best_k, risk, post
    def call(**kw):
        args = dict(dpair=f, hyp=f, hyp_len=f, n_hyp=f, score=f, scale=1.0, B=4, N=5, T=40, out=f,
                    out_len=f, best_k=f, risk=f, post=f)
        args.update(kw)
        return lib.ob_mbr_select(*args.values(), None)
    ptrs = ("dpair", "hyp", "hyp_len", "n_hyp", "score", "out", "out_len", "best_k", "risk", "post")
    for name in ptrs:
        assert call(**{name: None}) == NULL, name         # every call is otherwise valid
    assert call(N=0) == SHAPE and call(N=33) == SHAPE and call(T=4097) == SHAPE
    assert call(B=-1) == SHAPE and call(T=-1) == SHAPE
    for bad in (-1.0, -1e-300, math.inf, math.nan):
        assert call(scale=bad) == SHAPE, bad
    for name in ("score", "risk", "post"):                                        # 8-byte
        assert call(**{name: 0x3004}) == ALIGN, name
    for name in ("dpair", "hyp", "hyp_len", "n_hyp", "out", "out_len", "best_k"):
        assert call(**{name: 0x3002}) == ALIGN, name
    assert call(T=0, hyp=None, out=None, dpair=None) == NULL  # T == 0 frees hyp and out only
    assert call(B=0, **{k: None for k in ptrs}) == OK


def test_python_surface_on_cpu():
    import torch

    import onebit_asr
    from onebit_asr import edit, metrics
    from onebit_asr.infer import DECODERS, GraphedInference, encode_and_decode

    for name in ("edit_distance", "nbest_edit_distance", "nbest_oracle", "mbr_select"):
        assert getattr(onebit_asr, name) is getattr(edit, name), name
    assert onebit_asr.token_error_counts is metrics.token_error_counts
    assert onebit_asr.compute_wer_device is metrics.compute_wer_device
    assert DECODERS == ("greedy", "beam", "rescore", "attention")

    tok = torch.zeros(2, 4, dtype=torch.int32)
    ln = torch.tensor([4, 2], dtype=torch.int32)
    nbest = torch.zeros(2, 3, 4, dtype=torch.int32)
    nlen, nh = torch.zeros(2, 3, dtype=torch.int32), torch.tensor([3, 1], dtype=torch.int32)
    with pytest.raises(RuntimeError, match=r"edit_distance runs on the HIP library \(no CPU"):
        edit.edit_distance(tok, ln, tok, ln)
    with pytest.raises(RuntimeError, match=r"nbest_edit_distance runs on the HIP library \(no"):
        edit.nbest_edit_distance(nbest, nlen, nh, pairwise=True)
    with pytest.raises(RuntimeError, match=r"mbr_select runs on the HIP library \(no CPU"):
        edit.mbr_select(nbest, nlen, nh, torch.zeros(2, 3, dtype=torch.float64))
    with pytest.raises(RuntimeError, match=r"edit_distance runs on the HIP library \(no CPU"):
        metrics.token_error_counts(tok, ln, tok, ln)
    with pytest.raises(RuntimeError, match=r"edit_distance runs on the HIP library \(no CPU"):
        metrics.compute_wer_device(["a b"], ["a c"], "cpu")
    assert metrics.compute_wer_device([], [], "cpu") == (0, 0)
    for bad in (-0.5, math.inf, math.nan):
        with pytest.raises(ValueError, match="mbr_scale"):
            edit.mbr_select(nbest, nlen, nh, torch.zeros(2, 3), bad)

    # nbest_oracle is plain torch: ties to the smaller k, absent entries are -1
    dref = torch.tensor([[3, 1, 1, -1], [-1, -1, -1, -1], [0, 5, -1, -1]], dtype=torch.int32)
    best_k, dist = edit.nbest_oracle(dref)
    assert best_k.tolist() == [1, 0, 0] and dist.tolist() == [1, -1, 0]
    assert dist.dtype == torch.int32

    # mbr_scale: keyword only, default None, first after the marker and so ahead of
    # joint_ctc_weight / ctc_cand, which stay last
    for fn in (encode_and_decode, GraphedInference.__init__):
        p = inspect.signature(fn).parameters
        names = list(p)
        assert p["mbr_scale"].default is None
        assert p["mbr_scale"].kind is inspect.Parameter.KEYWORD_ONLY
        assert names.index("timestamps") + 1 == names.index("mbr_scale")
        assert names.index("mbr_scale") < names.index("joint_ctc_weight")
        assert names[-2:] == ["joint_ctc_weight", "ctc_cand"]
        assert p["timestamps"].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
    with pytest.raises(ValueError, match="mbr_scale needs decoder"):
        encode_and_decode(None, {}, mbr_scale=1.0)
    with pytest.raises(ValueError, match="mbr_scale needs decoder"):
        GraphedInference(torch.nn.Identity(), act_quant=None, mbr_scale=0.0)
    for bad in (-1.0, math.inf, math.nan):
        with pytest.raises(ValueError, match="mbr_scale must be >= 0 and finite"):
            encode_and_decode(None, {}, decoder="beam", mbr_scale=bad)
        with pytest.raises(ValueError, match="mbr_scale must be >= 0 and finite"):
            GraphedInference(torch.nn.Identity(), act_quant=None, decoder="rescore", mbr_scale=bad)
    g = GraphedInference(torch.nn.Identity(), act_quant=None, decoder="beam", mbr_scale=0)
    assert g.mbr_scale == 0.0 and isinstance(g.mbr_scale, float)
    assert GraphedInference(torch.nn.Identity(), act_quant=None, decoder="beam").mbr_scale is None
