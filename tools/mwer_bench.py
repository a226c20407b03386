#!/usr/bin/env python3
"""Minimum-WER loss timing at the Conformer-S shape (B = 32, T = 249, V = 5004, Th = 40,
N in {4, 10}) on a given n-best: ``mwer_ctc_loss`` forward and backward (csrc/ctcnbest.hip) next
to the composition that the entries before it allow, written here from those entries alone:

* the logits repeated N times ([B * N, T, V]);
* ``ctc_loss_logits_groups`` with one group per row (ll = -loss * max(L, 1)); the entry takes at
  most 64 groups, so the B * N rows go in chunks of 64;
* the posterior, the risk and the loss in float64 torch; autograd sums the dense [B * N, T, V]
  gradient over N.

The n-best: per utterance a random reference of 20..40 tokens and N entries a few edits away
from it; the logits are unit noise with a +3 peak along a uniform alignment of the reference
(blank between the tokens), ragged lengths. The two sides alternate in one run. HIP events
around the forward and around the backward of each call, after warm-up; median / min / max over
--reps calls; the losses and gradients of the two sides are compared. One JSON line.
Usage: python tools/mwer_bench.py [--reps 20] [--out profiles/r18/mwer_bench.json]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "cmu-11785-idl-1.58bit-asr_amd")]

import torch  # noqa: E402

from onebit_asr import _lib  # noqa: E402
from onebit_asr.ctc import ctc_loss_logits_groups  # noqa: E402
from onebit_asr.edit import nbest_edit_distance  # noqa: E402
from onebit_asr.mwer import mwer_ctc_loss  # noqa: E402

BLANK = 3


def make_inputs(B, T, V, Th, N, seed, dev):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, V, generator=g)
    lens = torch.randint(T // 2, T + 1, (B,), generator=g)
    lens[0] = T
    ref = torch.zeros(B, Th, dtype=torch.int64)
    ref_len = torch.randint(Th // 2, Th + 1, (B,), generator=g)
    hyp = torch.full((B, N, Th), -1, dtype=torch.int32)
    hyp_len = torch.zeros(B, N, dtype=torch.int32)
    for b in range(B):
        L = int(ref_len[b])
        r = torch.randint(4, V, (L,), generator=g)
        ref[b, :L] = r
        span = int(lens[b]) // L
        for u in range(L):  # token u peaks on the second half of its span, blank on the first
            x[b, u * span:u * span + span // 2, BLANK] += 3.0
            x[b, u * span + span // 2:(u + 1) * span, int(r[u])] += 3.0
        for k in range(N):
            e = r.tolist()
            for _ in range(k % 4):  # entry 0 is the reference; the others 1..3 edits away
                pos = int(torch.randint(0, len(e), (1,), generator=g))
                if int(torch.randint(0, 2, (1,), generator=g)) or len(e) < 2:
                    e[pos] = int(torch.randint(4, V, (1,), generator=g))
                else:
                    del e[pos]
            if k >= 4:  # keep the entries distinct
                e[k % len(e)] = 4 + (k * 7919) % (V - 4)
            hyp[b, k, :len(e)] = torch.tensor(e, dtype=torch.int32)
            hyp_len[b, k] = len(e)
    n_hyp = torch.full((B,), N, dtype=torch.int32)
    return [t.to(dev) for t in (x, lens, ref, ref_len, hyp, hyp_len, n_hyp)]


def naive(x, lens, hyp, hyp_len, err, scale):
    """The same loss from ctc_loss_logits_groups: logits repeated, one group per row."""
    B, N, Th = hyp.shape
    xr = x.repeat_interleave(N, dim=0)  # [B * N, T, V]
    tg = hyp.reshape(B * N, Th).to(torch.int64).clamp(min=0)
    il = lens.repeat_interleave(N)
    tl = hyp_len.reshape(B * N).to(torch.int64)
    parts = []
    for lo in range(0, B * N, 64):
        hi = min(lo + 64, B * N)
        parts.append(ctc_loss_logits_groups(xr[lo:hi], tg[lo:hi], il[lo:hi], tl[lo:hi], BLANK,
                                            hi - lo))
    ll = (-torch.cat(parts).double() * tl.clamp(min=1)).reshape(B, N)
    post = torch.softmax(scale * ll, dim=1)
    risk = (post * err).sum(dim=1)
    return (risk - err.mean(dim=1)).mean().float()


def stats(us):
    return {"median_us": round(statistics.median(us), 1), "min_us": round(min(us), 1),
            "max_us": round(max(us), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=249)
    ap.add_argument("--vocab", type=int, default=5004)
    ap.add_argument("--max-len", type=int, default=40)
    ap.add_argument("--nbest", type=int, nargs="+", default=[4, 10])
    ap.add_argument("--scale", type=float, default=0.5)
    ap.add_argument("--out", type=Path, default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _lib.load()
    B, T, V, Th = args.batch, args.frames, args.vocab, args.max_len
    st = torch.cuda.current_stream()
    res = {"device": torch.cuda.get_device_name(0), "digest": _lib.source_digest()[:12],
           "shape": dict(B=B, T=T, V=V, Th=Th), "reps": args.reps, "scale": args.scale,
           "cases": {}}
    for N in args.nbest:
        x, lens, ref, ref_len, hyp, hyp_len, n_hyp = make_inputs(B, T, V, Th, N, 0, dev)
        x.requires_grad_()
        err = nbest_edit_distance(hyp, hyp_len, n_hyp, ref, ref_len)["dref"].double()

        def new():
            return mwer_ctc_loss(x, lens, ref, ref_len, hyp, hyp_len, n_hyp, blank_id=BLANK,
                                 scale=args.scale)[0]

        def new_given():
            return mwer_ctc_loss(x, lens, None, None, hyp, hyp_len, n_hyp, blank_id=BLANK,
                                 scale=args.scale, errors=err)[0]

        def old():
            return naive(x, lens, hyp, hyp_len, err, args.scale)

        sides = {"mwer_ctc_loss": new, "mwer_ctc_loss_errors_given": new_given, "naive": old}
        check = {}
        for name, fn in sides.items():
            for _ in range(args.warmup):
                x.grad = None
                fn().backward()
            check[name] = (fn().detach(), x.grad.clone())
        torch.cuda.synchronize()
        times = {name: ([], []) for name in sides}
        for _ in range(args.reps):  # the sides alternate
            for name, fn in sides.items():
                x.grad = None
                e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                e[0].record(st)
                loss = fn()
                e[1].record(st)
                loss.backward()
                e[2].record(st)
                torch.cuda.synchronize()
                times[name][0].append(e[0].elapsed_time(e[1]) * 1e3)
                times[name][1].append(e[1].elapsed_time(e[2]) * 1e3)
        l_new, g_new = check["mwer_ctc_loss"]
        l_old, g_old = check["naive"]
        case = {name: {"forward": stats(f), "backward": stats(b),
                       "total_median_us": round(statistics.median(
                           [p + q for p, q in zip(f, b)]), 1)}
                for name, (f, b) in times.items()}
        case["loss"] = {"mwer_ctc_loss": l_new.item(), "naive": l_old.item()}
        case["grad_max_abs"] = g_old.abs().max().item()
        case["grad_max_diff"] = (g_new - g_old).abs().max().item()
        case["workspace_bytes"] = {
            "mwer_ctc_loss": lib.ob_ctc_nbest_workspace(B, N, T, Th),
            "naive_ctc_workspaces": sum(lib.ob_ctc_logits_workspace(min(64, B * N - lo), T, Th)
                                        for lo in range(0, B * N, 64)),
            "naive_repeated_logits_and_gradient": 2 * 4 * B * N * T * V}
        case["speedup_total"] = round(case["naive"]["total_median_us"]
                                      / case["mwer_ctc_loss"]["total_median_us"], 2)
        res["cases"][f"N={N}"] = case
        del check, g_new, g_old
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out is not None:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text(line + "\n")


if __name__ == "__main__":
    main()
