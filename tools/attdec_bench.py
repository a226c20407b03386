#!/usr/bin/env python3
"""Attention-decoder beam search timing at the inference batch (B = 256, T' = 249, V = 5004,
d = 144, N = 10 beam slots, L = 64 static steps, ragged memory lengths). HIP events around each
call on the launch stream, after warm-up; the median and the spread over --reps calls. Reports,
as one JSON line:

* the KV-cached search (``attention_beam_search``: ``ob_decattn_step`` + grouped cross-attention
  + ``ob_seq_topk`` + ``ob_attdec_beam_step`` per step), eager and replayed from a captured
  graph, next to the same search WITHOUT a cache, written here from existing code:
  ``TransformerDecoder.hidden`` on the growing prefix, then torch ``linear -> log_softmax ->
  topk`` over the [R, V] logits and torch gathers for the beam reorder (fewer reps: it is slow);
  and the share of utterances on which both return the same best hypothesis;
* the output layer with top-k (``ob_seq_topk``, K = N) next to that unfused torch expression on
  the same hidden rows, with the workspace next to the bytes of the [R, V] logits;
* the whole captured forward (Conformer-S, int8 activations) with ``decoder="attention"`` next
  to ``"beam"`` and ``"rescore"`` (the CTC blank bias is shifted as in rescore_bench.py so that
  the rescoring pass has hypotheses that fit max_len).
Usage: python tools/attdec_bench.py [--reps 20] [--skip-forward]"""
import argparse
import json
import sys
from pathlib import Path
from types import SimpleNamespace

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "cmu-11785-idl-1.58bit-asr_amd"), str(ROOT / "tools")]

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from decode_bench import ctc_like_logits, timed  # noqa: E402
from onebit_asr import _lib  # noqa: E402
from onebit_asr.attdec import attention_beam_search, seq_topk  # noqa: E402
from onebit_asr.conformer import ConformerASR, TransformerDecoder  # noqa: E402
from onebit_asr.data import CONFORMER_S, synthetic_batch  # noqa: E402
from onebit_asr.infer import GraphedInference  # noqa: E402

PAD, BOS, EOS, BLANK = 0, 1, 2, 3


@torch.no_grad()
def uncached_search(dec, mem, mask, n, steps):
    """The same search without a cache, from existing code (fp32 scores): every step runs the
    whole decoder on the prefixes so far and materialises the [R, V] log-probabilities."""
    b = mem.shape[0]
    dev = mem.device
    v = dec.out.weight.shape[0]
    inp = torch.full((b * n, 1), BOS, dtype=torch.long, device=dev)
    score = torch.full((b, n), -float("inf"), device=dev)
    score[:, 0] = 0.0
    fin = torch.zeros((b, n), dtype=torch.bool, device=dev)
    for t in range(steps):
        pad = torch.zeros(inp.shape, dtype=torch.bool, device=dev)
        h = dec.hidden(inp, mem, mask, pad, mem_group=n)[:, -1]
        lp = torch.log_softmax(F.linear(h, dec.out.weight, dec.out.bias), dim=-1).view(b, n, v)
        lp[..., [PAD, BOS, BLANK]] = -float("inf")
        carry = torch.full_like(lp, -float("inf"))
        carry[..., EOS] = 0.0                          # a finished slot: itself, unchanged
        cand = score.unsqueeze(-1) + torch.where(fin.unsqueeze(-1), carry, lp)
        score, idx = cand.view(b, n * v).topk(n, dim=-1)
        par, tok = idx // v, idx % v
        rows = (par + torch.arange(b, device=dev).unsqueeze(1) * n).view(-1)
        was_fin = fin.view(-1)[rows].view(b, n)
        fin = was_fin | (tok == EOS)
        nxt = torch.where(fin, torch.tensor(PAD, device=dev), tok).view(-1, 1)
        inp = torch.cat([inp[rows], nxt], dim=1)
    return inp.view(b, n, steps + 1)[:, :, 1:], score


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--frames", type=int, default=249)
    ap.add_argument("--vocab", type=int, default=5004)
    ap.add_argument("--beam", type=int, default=10)
    ap.add_argument("--max-len", type=int, default=64)
    ap.add_argument("--skip-forward", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _lib.load()
    B, T, V, N, L = args.batch, args.frames, args.vocab, args.beam, args.max_len
    d = CONFORMER_S["enc_d_model"]
    res = {}

    def note(msg):
        print(msg, file=sys.stderr, flush=True)

    # 1. the search, cached and not: seeded memory, ragged masks
    _, lens = ctc_like_logits(B, T, 16, 3, 0, dev)  # (only the ragged lengths are used)
    torch.manual_seed(0)
    dec = TransformerDecoder(V, d, CONFORMER_S["dec_layers"], CONFORMER_S["dec_heads"],
                             CONFORMER_S["dec_d_ff"], 0.1, 0).to(dev).eval()
    model = SimpleNamespace(decoder=dec)
    g = torch.Generator().manual_seed(1)
    mem = torch.randn(B, T, d, generator=g).to(dev)
    mask = (torch.arange(T)[None, :] < lens.cpu().clamp(min=1)[:, None]).to(dev)
    res["search_cached_eager"] = timed(lambda: attention_beam_search(model, mem, mask, N, L),
                                       args.reps, args.warmup)
    note(f"search_cached_eager {res['search_cached_eager']}")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = attention_beam_search(model, mem, mask, N, L)
    res["search_cached_graph"] = timed(graph.replay, args.reps, args.warmup)
    note(f"search_cached_graph {res['search_cached_graph']}")
    res["search_uncached_torch"] = timed(lambda: uncached_search(dec, mem, mask, N, L),
                                         max(3, args.reps // 4), 1)
    note(f"search_uncached_torch {res['search_uncached_torch']}")
    graph.replay()
    hyp, hyp_len = out[0], out[1]
    ref, _ = uncached_search(dec, mem, mask, N, L)
    pos = torch.arange(L, device=dev)[None, :]
    same = (torch.where(pos < hyp_len[:, :1], hyp[:, 0].long(), torch.tensor(0, device=dev)) ==
            torch.where(pos < hyp_len[:, :1], ref[:, 0], torch.tensor(0, device=dev))).all(dim=1)
    res["best_hypothesis_equal_share"] = round(float(same.float().mean().item()), 3)
    res["best_hyp_len_mean"] = round(float(hyp_len[:, 0].float().mean().item()), 1)
    res["cache_bytes"] = len(dec.dec.layers) * L * B * N * 2 * d * 4
    del graph, out

    # 2. the output layer with top-k, fused and unfused, on R = B * N hidden rows
    rows = B * N
    with torch.no_grad():
        h = torch.randn(rows, d, generator=g).to(dev)
        w, bias = dec.out.weight.detach(), dec.out.bias.detach()
        banned = (PAD, BOS, BLANK)
        res["topk_fused"] = timed(lambda: seq_topk(h, w, bias, N, banned), args.reps, args.warmup)

        def unfused():
            lsm = torch.log_softmax(F.linear(h, w, bias), dim=-1)
            lsm[:, list(banned)] = -float("inf")
            return lsm.topk(N, dim=-1)

        res["topk_unfused_torch"] = timed(unfused, args.reps, args.warmup)
        lse, topv, topi = seq_topk(h, w, bias, N, banned)
        uv, ui = unfused()
        res["topk_index_equal_share"] = round(float((topi.long() == ui).float().mean().item()), 5)
        res["topk_max_abs_diff"] = float(((topv.double() - lse[:, None]) - uv.double()).abs()
                                         .max().item())
    res["topk_workspace_bytes"] = lib.ob_seq_topk_workspace(rows, d, V, N)
    res["unfused_logits_bytes"] = rows * V * 4
    del h, mem

    # 3. the whole forward, captured
    fwd = {}
    if not args.skip_forward:
        torch.manual_seed(0)
        full = ConformerASR(80, V, **CONFORMER_S).to(dev).eval()
        batch = synthetic_batch([1000] * B, [40] * B, seed=1234, device=dev)
        batch["feat_lens"] = (lens * 4).clamp(max=1000).to(dev)
        with torch.no_grad():
            _, _, lg = full(batch, precision=2)
            others = lg.clone()
            others[..., 3] = -float("inf")
            gap = (others.max(dim=-1).values - lg[..., 3]).flatten()
            full.ctc_head.bias[3] += torch.quantile(gap[:1 << 20].float(), 0.85)
            del lg, others, gap
        for name in ("beam", "rescore", "attention"):
            gi = GraphedInference(full, precision=2, decoder=name, beam_size=N, max_len=L)
            gi.run(batch)
            fwd["forward_" + name] = timed(lambda: gi.run(batch), max(3, args.reps // 2), 1)
            note(f"forward_{name} {fwd['forward_' + name]}")
            del gi
    print(json.dumps({"tool": "attdec_bench", "device": torch.cuda.get_device_name(0), "B": B,
                      "T": T, "V": V, "d": d, "beam": N, "max_len": L, "rows": rows,
                      "reps": args.reps, **res, **fwd, "digest": _lib.source_digest()[:12]}))


if __name__ == "__main__":
    main()
