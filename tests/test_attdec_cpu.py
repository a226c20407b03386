"""CPU: the oracle of the attention-decoder beam search (tests/attdec_ref.py) against answers
derived by hand (tests/golden/attdec_bookkeeping.json) and against a plain argmax loop; the
argument checks of the new C entry points, which fail before any HIP call; the Python surface's
decoder switch."""
import json
import math
from pathlib import Path

import numpy as np
import pytest

import attdec_ref as ar

GOLDEN = json.loads((Path(__file__).parent / "golden" / "attdec_bookkeeping.json").read_text())


def _score(x):
    return -math.inf if x is None else x


@pytest.mark.parametrize("case", GOLDEN["cases"], ids=[c["name"] for c in GOLDEN["cases"]])
def test_bookkeeping_by_hand(case):
    res = ar.beam_search(ar.table_logp(case["table"], case["default"]), case["N"], case["L"],
                         case["alpha"], GOLDEN["special"])
    assert res.hyps == case["hyps"]
    assert res.scores == case["scores"] and res.finished == case["finished"]
    want = [[(p, v, _score(s)) for p, v, s in row] for row in case["trace"]]
    assert res.trace == want


def test_golden_cases_cover_what_they_claim():
    cases = {c["name"]: c for c in GOLDEN["cases"]}
    tie = ar.beam_search(ar.table_logp(cases["tie_goes_to_the_smaller_slot_then_the_smaller_token"]
                                       ["table"], [0.0] + [-9.0] * 4), 3, 2, 0.0, GOLDEN["special"])
    assert tie.margin == 0.0                      # an exact tie decided the selection
    few = cases["fewer_candidates_than_slots"]
    assert few["trace"][0][-1] == [-1, ar.DEAD, None]
    a0 = cases["length_penalty_zero_prefers_the_short_hypothesis"]
    a1 = cases["length_penalty_one_prefers_the_long_hypothesis"]
    assert a0["table"] == a1["table"] and a0["hyps"][0] != a1["hyps"][0]
    done = cases["every_slot_finished_before_the_last_step"]
    assert all(v == ar.CARRIED for row in done["trace"][2:] for _, v, _ in row)
    # an utterance without a valid frame has no hypothesis at all
    dead = ar.beam_search(lambda p: pytest.fail("no row is live"), 3, 2, alive=False)
    assert dead.hyps == [] and all(v == ar.DEAD for row in dead.trace for _, v, _ in row)


def test_greedy_oracle_is_an_argmax_loop_without_a_cache():
    """N = 1: the oracle on the model wrapper (no cache) equals a plain loop over
    ``model64.decode_logits`` that appends the best non-special token until eos."""
    import torch

    import rescore_ref as rr
    from onebit_asr.conformer import ConformerASR
    from onebit_asr.data import CFG1

    torch.manual_seed(0)
    model64 = rr.double_model(ConformerASR(80, 40, **CFG1))
    g = torch.Generator().manual_seed(5)
    enc = torch.randn(2, 30, 64, generator=g, dtype=torch.float64)
    mask = torch.ones(2, 30, dtype=torch.long)
    mask[1, 11:] = 0
    L = 6
    with torch.no_grad():
        model64.decoder.out.bias[2] += 1.0   # make eos reachable inside L steps
    for b in range(2):
        res = ar.beam_search(ar.model_logp(model64, enc[b].numpy(), mask[b].numpy()), 1, L)
        toks, score, fin = [], 0.0, False
        for _ in range(L):
            inp = torch.tensor([[1] + toks])
            with torch.no_grad():
                z = model64.decode_logits(enc[b:b + 1], mask[b:b + 1], inp,
                                          torch.zeros(inp.shape, dtype=torch.bool))
            lp = torch.log_softmax(z[0, -1], dim=-1)
            lp_c = lp.clone()
            lp_c[[0, 1, 3]] = -math.inf
            v = int(lp_c.argmax())
            score += float(lp[v])
            if v == 2:
                fin = True
                break
            toks.append(v)
        assert res.hyps == [toks] and res.finished == [fin]
        assert abs(res.scores[0] - score) <= 1e-12
        assert len(res.trace) == L and res.margin > 0


def test_new_entries_reject_bad_arguments_without_gpu():
    """Every check below fails before any HIP call, so it is safe with no device."""
    from onebit_asr import _lib

    lib = _lib.load()
    f = 0x1000
    big = 1 << 30
    NULL, SHAPE, WS, ALIGN = -1, -2, -4, -5
    # limits: N, d, H, Lk, L
    sup = lib.ob_attdec_supported
    assert sup(10, 144, 4, 249, 64) and sup(1, 64, 4, 1, 1) and sup(32, 256, 4, 256, 255)
    assert not sup(33, 144, 4, 249, 64) and not sup(0, 144, 4, 249, 64)    # N
    assert not sup(10, 80, 4, 249, 64)                                     # dh = 20
    assert not sup(10, 144, 4, 249, 256)                                   # L + 1 > 256
    assert not sup(10, 72, 2, 249, 64)                                     # d % 16 != 0
    assert not sup(10, 144, 4, 257, 64) and not sup(10, 144, 4, 249, 0)    # Lk, L
    # step attention: qkv, sq, cache, anc, skip, R, H, dh, L, t, ctx
    sa = lib.ob_decattn_step
    assert sa(f, 192, f, f, None, 6, 4, 20, 12, 3, f, None) == SHAPE       # dh = 20
    assert sa(f, 192, f, f, None, 6, 4, 16, 256, 3, f, None) == SHAPE      # L + 1 > 256
    assert sa(f, 192, f, f, None, 6, 4, 16, 12, 12, f, None) == SHAPE      # t >= L
    assert sa(f, 190, f, f, None, 6, 4, 16, 12, 3, f, None) == SHAPE       # sq < 3 H dh
    assert sa(f, 194, f, f, None, 6, 4, 16, 12, 3, f, None) == SHAPE       # sq % 4
    assert sa(None, 192, f, f, None, 6, 4, 16, 12, 3, f, None) == NULL
    assert sa(f, 192, f, None, None, 6, 4, 16, 12, 3, f, None) == NULL     # anc
    assert sa(0x1004, 192, f, f, None, 6, 4, 16, 12, 3, f, None) == ALIGN  # qkv rows: 16 bytes
    assert sa(f, 192, 0x1008, f, None, 6, 4, 16, 12, 3, f, None) == ALIGN  # cache
    assert sa(f, 192, f, 0x1002, None, 6, 4, 16, 12, 3, f, None) == ALIGN
    assert sa(None, 192, None, None, None, 0, 4, 16, 12, 3, None, None) == 0   # R == 0
    # top-k output layer: hidden, R, d, W, bias, V, banned, n_banned, skip, K, ws, bytes, lse, v, i
    tk = lib.ob_seq_topk
    assert tk(f, 4, 20, f, f, 5, None, 0, None, 2, f, big, f, f, f, None) == SHAPE    # d % 16
    assert tk(f, 4, 272, f, f, 5, None, 0, None, 2, f, big, f, f, f, None) == SHAPE   # d > 256
    assert tk(f, 4, 16, f, f, 5, None, 0, None, 33, f, big, f, f, f, None) == SHAPE   # K > 32
    assert tk(f, 4, 16, f, f, 5, None, 0, None, 0, f, big, f, f, f, None) == SHAPE
    assert tk(f, 4, 16, f, f, 5, None, 9, None, 2, f, big, f, f, f, None) == SHAPE    # n_banned
    assert tk(None, 4, 16, f, f, 5, None, 0, None, 2, f, big, f, f, f, None) == NULL
    assert tk(f, 4, 16, f, f, 5, None, 2, None, 2, f, big, f, f, f, None) == NULL     # banned
    assert tk(f, 4, 16, f, f, 5, None, 0, None, 2, f, big, None, f, f, None) == NULL  # lse
    assert tk(0x1004, 4, 16, f, f, 5, None, 0, None, 2, f, big, f, f, f, None) == ALIGN
    assert tk(f, 4, 16, f, f, 5, None, 0, None, 2, f, big, 0x1004, f, f, None) == ALIGN  # fp64
    assert tk(f, 4, 16, f, f, 5, None, 0, None, 2, 0x1004, big, f, f, f, None) == ALIGN
    assert lib.ob_seq_topk_workspace(4, 20, 5, 2) == 0
    assert lib.ob_seq_topk_workspace(4, 16, 5, 33) == 0
    need = lib.ob_seq_topk_workspace(130, 144, 5004, 10)
    print(f"ob_seq_topk_workspace(130, 144, 5004, 10) = {need} bytes; the [R][V] logits would be "
          f"{130 * 5004 * 4}")
    assert 0 < need < 130 * 5004 * 4
    assert lib.ob_seq_topk_workspace(130, 144, 5004, 32) < 130 * 5004 * 4
    assert tk(f, 130, 144, f, f, 5004, None, 0, None, 10, f, need - 1, f, f, f, None) == WS
    assert tk(f, 0, 144, f, f, 5004, None, 0, None, 10, None, 0, None, None, None, None) == 0
    # init: kmask, B, N, Lk, L, bos, score, len, fin, tok, skip, anc
    ini = lib.ob_attdec_init
    assert ini(f, 2, 33, 9, 12, 1, f, f, f, f, f, f, None) == SHAPE        # N > 32
    assert ini(f, 2, 4, 9, 256, 1, f, f, f, f, f, f, None) == SHAPE        # L + 1 > 256
    assert ini(f, 2, 4, 0, 12, 1, f, f, f, f, f, f, None) == SHAPE
    assert ini(f, 2, 4, 9, 12, 1, None, f, f, f, f, f, None) == NULL
    assert ini(f, 2, 4, 9, 12, 1, f, f, f, f, f, None, None) == NULL
    assert ini(f, 2, 4, 9, 12, 1, 0x1004, f, f, f, f, f, None) == ALIGN    # fp64 score
    assert ini(f, 2, 4, 9, 12, 1, f, f, f, 0x1004, f, f, None) == ALIGN    # int64 tok
    assert ini(None, 0, 4, 9, 12, 1, None, None, None, None, None, None, None) == 0  # B == 0
    # beam step: lse, topv, topi, B, N, K, L, t, eos, pad, norm, anc_in, anc_out, score, len, fin,
    #            tok, skip, trace_parent, trace_token, trace_score
    bs = lib.ob_attdec_beam_step
    g = 0x2000
    assert bs(f, f, f, 2, 33, 4, 12, 0, 2, 0, f, f, g, f, f, f, f, f, f, f, f, None) == SHAPE
    assert bs(f, f, f, 2, 4, 33, 12, 0, 2, 0, f, f, g, f, f, f, f, f, f, f, f, None) == SHAPE
    assert bs(f, f, f, 2, 4, 4, 12, 12, 2, 0, f, f, g, f, f, f, f, f, f, f, f, None) == SHAPE
    assert bs(f, f, f, 2, 4, 4, 256, 0, 2, 0, f, f, g, f, f, f, f, f, f, f, f, None) == SHAPE
    assert bs(f, f, f, 2, 4, 4, 12, 0, 2, 0, f, f, f, f, f, f, f, f, f, f, f, None) == SHAPE  # in = out
    assert bs(None, f, f, 2, 4, 4, 12, 0, 2, 0, f, f, g, f, f, f, f, f, f, f, f, None) == NULL
    assert bs(f, f, f, 2, 4, 4, 12, 0, 2, 0, None, f, g, f, f, f, f, f, f, f, f, None) == NULL
    assert bs(f, f, f, 2, 4, 4, 12, 0, 2, 0, f, f, g, f, f, f, f, f, f, f, None, None) == NULL
    assert bs(0x1004, f, f, 2, 4, 4, 12, 0, 2, 0, f, f, g, f, f, f, f, f, f, f, f, None) == ALIGN
    assert bs(f, f, f, 2, 4, 4, 12, 0, 2, 0, f, f, g, f, f, f, f, f, f, f, 0x1004, None) == ALIGN
    assert bs(f, f, 0x1002, 2, 4, 4, 12, 0, 2, 0, f, f, g, f, f, f, f, f, f, f, f, None) == ALIGN
    assert bs(*([None] * 3), 0, 4, 4, 12, 0, 2, 0, *([None] * 11), None) == 0   # B == 0
    # finalize: trace_parent, trace_token, score, len, fin, B, N, L, eos, hyp, hyp_len, n_hyp,
    #           score_out, finished
    fz = lib.ob_attdec_finalize
    assert fz(f, f, f, f, f, 2, 0, 12, 2, f, f, f, f, f, None) == SHAPE
    assert fz(f, f, f, f, f, 2, 4, 0, 2, f, f, f, f, f, None) == SHAPE
    assert fz(None, f, f, f, f, 2, 4, 12, 2, f, f, f, f, f, None) == NULL
    assert fz(f, f, f, f, f, 2, 4, 12, 2, f, f, f, f, None, None) == NULL
    assert fz(f, f, 0x1004, f, f, 2, 4, 12, 2, f, f, f, f, f, None) == ALIGN
    assert fz(f, f, f, f, f, 2, 4, 12, 2, f, f, f, 0x1004, f, None) == ALIGN
    assert fz(f, f, f, f, f, 2, 4, 12, 2, 0x1002, f, f, f, f, None) == ALIGN
    assert fz(*([None] * 5), 0, 4, 12, 2, *([None] * 5), None) == 0   # B == 0


def test_decoder_switch_accepts_attention():
    from onebit_asr.infer import DECODERS, GraphedInference, encode_and_decode

    assert DECODERS == ("greedy", "beam", "rescore", "attention")
    with pytest.raises(ValueError, match="decoder must be"):
        encode_and_decode(None, {}, decoder="bogus")
    import torch

    gi = GraphedInference(torch.nn.Identity(), act_quant=None, decoder="attention", beam_size=4,
                          max_len=12, length_penalty=0.6)
    assert (gi.decoder, gi.beam_size, gi.max_len, gi.length_penalty) == ("attention", 4, 12, 0.6)


def test_python_surface_on_cpu():
    import torch

    import onebit_asr
    from onebit_asr.attdec import attention_beam_search, decattn_step, length_norm, seq_topk
    from onebit_asr.conformer import ConformerASR
    from onebit_asr.data import CFG1
    from onebit_asr.infer import encode_and_decode

    assert onebit_asr.attention_beam_search is attention_beam_search
    assert callable(onebit_asr.attention_decode_batch) and onebit_asr.seq_topk is seq_topk
    torch.manual_seed(0)
    model = ConformerASR(80, 40, **CFG1).eval()
    enc, mask = torch.zeros(2, 9, 64), torch.ones(2, 9, dtype=torch.long)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        attention_beam_search(model, enc, mask, beam_size=4, max_len=8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        onebit_asr.attention_decode_batch(model, enc, mask, beam_size=4, max_len=8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        seq_topk(torch.zeros(2, 16), torch.zeros(5, 16), None, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        decattn_step(torch.zeros(2, 48), torch.zeros(4, 2, 32), torch.zeros(2, 4, dtype=torch.int32),
                     None, 1, 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.decoder.new_cache(enc, mask, 4, 8)
    # the switch reaches the search: a CPU batch (full-precision encoder, which runs on the
    # CPU) gets as far as the search's own no-CPU-fallback error
    from onebit_asr.data import synthetic_batch

    batch = synthetic_batch([61], [3], vocab=40, device="cpu")
    with pytest.raises(RuntimeError, match="attention_beam_search runs on the HIP library"):
        encode_and_decode(model, batch, precision=32, decoder="attention", beam_size=2, max_len=4)
    # the length normaliser: max(n, 1) ** alpha in float64
    assert length_norm(3, 0.0).tolist() == [1.0, 1.0, 1.0, 1.0]
    assert length_norm(3, 0.5).tolist() == [1.0, 1.0, 2.0 ** 0.5, 3.0 ** 0.5]
    assert length_norm(3, 0.5).dtype == torch.float64
