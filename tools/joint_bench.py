#!/usr/bin/env python3
"""Joint CTC/attention beam search timing at attdec_bench.py's shape (B = 256, T' = 249,
V = 5004, d = 144, N = 10 beam slots, L = 64 static steps, K = 20 attention candidates per slot,
w = 0.3, ragged memory lengths). HIP events around each call on the launch stream, after
warm-up; the median and the spread over --reps calls. Reports, as one JSON line:

* ``joint_beam_search`` eager and replayed from a captured graph, next to
  ``attention_beam_search`` on the same memory in the same run, with the mean length and the
  finished share of the best hypotheses of both;
* the frame log-sum-exp launch (``ob_ctc_frame_lse``, once per search);
* the prefix scorer step (``ob_ctc_prefix_step``) on the search's own state at steps 0, 31 and
  63 (the tool drives the search's phases itself and repeats one there), with the live rows of
  each, next to ``ob_seq_topk`` at K = 20 and the joint beam step (``ob_attdec_joint_step``) at
  the same steps;
* the state workspace in bytes (``ob_ctc_prefix_workspace``: the same for every K).
Usage: python tools/joint_bench.py [--reps 20]"""
import argparse
import json
import sys
from pathlib import Path
from types import SimpleNamespace

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "cmu-11785-idl-1.58bit-asr_amd"), str(ROOT / "tools")]

import torch  # noqa: E402

from decode_bench import ctc_like_logits, timed  # noqa: E402
from onebit_asr import _lib  # noqa: E402
from onebit_asr.attdec import (SPECIAL, _BeamSearch, attention_beam_search,  # noqa: E402
                               ctc_frame_lse, joint_beam_search, seq_topk)
from onebit_asr.conformer import TransformerDecoder  # noqa: E402
from onebit_asr.data import CONFORMER_S  # noqa: E402

PAD, BOS, EOS, BLANK = 0, 1, 2, 3


@torch.no_grad()
def stepwise(model, enc, mask, z, n, k, L, w, keep, reps, warmup):
    """The joint search, phase by phase (``attdec._BeamSearch``); at the steps in ``keep`` the
    scorer step, the top-k output layer and the joint beam step are timed on the state the search
    has there."""
    bs = _BeamSearch(model, enc, mask, n, k, L, 0.0, SPECIAL, z, w)
    assert bs.mode.ctc, "--weight must be > 0: the CTC scorer is timed"
    st, dec = bs.state, model.decoder
    rewritten = ("score", "att", "ctc", "length", "fin", "tok", "skip", "link")
    out = {}
    for t in range(L):
        bs.propose(t)
        bs.score_ctc(t)
        if t in keep:
            out[f"scorer_step_t{t}"] = timed(lambda: bs.score_ctc(t), reps, warmup)
            out[f"seq_topk_k{k}_t{t}"] = timed(
                lambda: seq_topk(bs.hidden, dec.out.weight, dec.out.bias, k, bs.banned, st["skip"],
                                 st["cand"]), reps, warmup)
            # the beam step rewrites the state: time it on copies
            copies = bs.clone_state(rewritten)

            def copies_only():
                for name in rewritten:
                    copies[name].copy_(st[name])

            def on_copies():
                copies_only()
                bs.select(t, copies)

            both, base = timed(on_copies, reps, warmup), timed(copies_only, reps, warmup)
            out[f"joint_step_t{t}"] = {"median_us": round(both["median_us"] - base["median_us"], 1),
                                       "with_state_copies_us": both["median_us"]}
            out[f"live_rows_t{t}"] = int((st["skip"] == 0).sum().item())
            out[f"finite_cpsi_share_t{t}"] = round(float(
                torch.isfinite(st["cpsi"][st["skip"] == 0]).float().mean().item()), 3)
        bs.select(t)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--frames", type=int, default=249)
    ap.add_argument("--vocab", type=int, default=5004)
    ap.add_argument("--beam", type=int, default=10)
    ap.add_argument("--cand", type=int, default=20)
    ap.add_argument("--max-len", type=int, default=64)
    ap.add_argument("--weight", type=float, default=0.3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _lib.load()
    B, T, V, N, K, L, w = (args.batch, args.frames, args.vocab, args.beam, args.cand,
                           args.max_len, args.weight)
    d = CONFORMER_S["enc_d_model"]
    res = {}

    def note(msg):
        print(msg, file=sys.stderr, flush=True)

    z, lens = ctc_like_logits(B, T, V, BLANK, 0, dev)   # CTC-like logits, ragged lengths
    torch.manual_seed(0)
    dec = TransformerDecoder(V, d, CONFORMER_S["dec_layers"], CONFORMER_S["dec_heads"],
                             CONFORMER_S["dec_d_ff"], 0.1, 0).to(dev).eval()
    model = SimpleNamespace(decoder=dec)
    g = torch.Generator().manual_seed(1)
    mem = torch.randn(B, T, d, generator=g).to(dev)
    mask = (torch.arange(T)[None, :] < lens.cpu().clamp(min=1)[:, None]).to(dev)

    def summary(out):
        hyp_len, n_hyp, fin = out[1], out[2], out[4]["finished"]
        return {"best_hyp_len_mean": round(float(hyp_len[:, 0].float().mean().item()), 1),
                "best_finished_share": round(float(fin[:, 0].float().mean().item()), 3),
                "n_hyp_mean": round(float(n_hyp.float().mean().item()), 2)}

    searches = {"attention": lambda: attention_beam_search(model, mem, mask, N, L),
                "joint": lambda: joint_beam_search(model, mem, mask, z, N, L, w, K)}
    for name, fn in searches.items():
        res[f"search_{name}_eager"] = timed(fn, args.reps, args.warmup)
        note(f"search_{name}_eager {res[f'search_{name}_eager']}")
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = fn()
        res[f"search_{name}_graph"] = timed(graph.replay, args.reps, args.warmup)
        note(f"search_{name}_graph {res[f'search_{name}_graph']}")
        graph.replay()
        torch.cuda.synchronize()
        res[f"search_{name}_result"] = summary(out)
        del graph, out
    for kind in ("eager", "graph"):
        a, j = res[f"search_attention_{kind}"]["median_us"], res[f"search_joint_{kind}"]["median_us"]
        res[f"joint_over_attention_{kind}"] = round(j / a, 3)
        res[f"per_step_us_{kind}"] = {"attention": round(a / L, 1), "joint": round(j / L, 1)}

    lens64 = mask.sum(dim=1).to(torch.int64).contiguous()
    flse = torch.empty((B, T), dtype=torch.float64, device=dev)
    res["frame_lse"] = timed(lambda: ctc_frame_lse(z, lens64, flse), args.reps, args.warmup)
    res.update(stepwise(model, mem, mask, z, N, K, L, w, (0, L // 2 - 1, L - 1), args.reps,
                        args.warmup))
    res["state_workspace_bytes"] = lib.ob_ctc_prefix_workspace(B, N, K, T)
    res["state_workspace_bytes_k32"] = lib.ob_ctc_prefix_workspace(B, N, 32, T)
    res["state_per_candidate_would_be_bytes"] = 2 * B * N * K * T * 2 * 8
    print(json.dumps({"tool": "joint_bench", "device": torch.cuda.get_device_name(0), "B": B,
                      "T": T, "V": V, "d": d, "beam": N, "cand": K, "max_len": L, "weight": w,
                      "rows": B * N, "reps": args.reps, **res,
                      "digest": _lib.source_digest()[:12]}))


if __name__ == "__main__":
    main()
