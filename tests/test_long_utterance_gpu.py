"""Utterances past the fused attention kernels' 512 subsampled frames stay on the device under
no_grad: MHSA routes their attention core to the forward-only key-chunk kernel
(attention.rel_pos_attention_infer, csrc/relattn_long.hip) with the projections and epilogues
of the short path around it.

A small ConformerASR (80 mel bins, d_model 64, 4 heads of 16, 2 blocks, d_ff 128, conv kernel 31,
32-entry vocabulary, dropout 0.1 so that train mode has an effective dropout) in eval mode on a
padded batch of 2100, 2055 and 900 frames: padded T' = 524, valid frames 524, 513 and 225 (the
model's mask keeps feat_lens // 4 frames).

* logits at precision 2 and 32 against the CPU oracle built from the same state dict, at
  tests/test_model_gpu.py's CTC-logit bar (max |err| <= 1e-3), with a wrapper counting exactly
  one rel_pos_attention_infer call per block (without the count the torch fallback would pass);
* greedy and beam decode of that batch return counts within lens;
* GraphedInference replays to logits within 1e-4 * max|logit| of the eager run
  (tests/test_infer_gpu.py's bar for the same comparison);
* routing negatives, the wrapper's count staying 0: grad mode on, train mode with dropout 0.1
  under no_grad, OB_ATTN=torch (each equal, torch.equal, to a direct run of the torch path) and
  T' <= 512 (rel_pos_attention, i.e. ob_relattn_fwd, runs once per block instead);
* the int8-activation model: one call per block and finite logits (its activations are
  re-quantised after the core, so no numeric bar is set for it).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

N_BLOCKS = 2
VOCAB = 32
CFG = dict(enc_d_model=64, enc_layers=N_BLOCKS, enc_heads=4, enc_d_ff=128, enc_conv_kernel=31,
           enc_dropout=0.1, dec_layers=2, dec_heads=4, dec_d_ff=128, dec_dropout=0.1)
CFG_ORACLE = dict(input_dim=80, vocab_size=VOCAB, d_model=64, n_layers=N_BLOCKS, n_heads=4,
                  d_ff=128, conv_kernel=31, dec_layers=2, dec_heads=4, dec_d_ff=128, dropout=0.0)
FRAMES = [2100, 2055, 900]
SUB_LENS = [524, 513, 225]   # valid subsampled frames (feat_lens // 4, at most the padded 524)


@pytest.fixture(scope="module")
def model(gpu):
    from onebit_asr.conformer import ConformerASR

    torch.manual_seed(0)
    return ConformerASR(80, VOCAB, **CFG).to(gpu).eval()


@pytest.fixture(scope="module")
def batch():
    from onebit_asr.data import synthetic_batch

    return synthetic_batch(FRAMES, [20, 20, 9], vocab=VOCAB, seed=0)


def _to(b, dev):
    return {k: v.to(dev) for k, v in b.items()}


class Counter:
    def __init__(self, fn):
        self.fn = fn
        self.n = 0

    def __call__(self, *a, **kw):
        self.n += 1
        return self.fn(*a, **kw)


@pytest.fixture
def infer_calls(monkeypatch):
    from onebit_asr import attention

    c = Counter(attention.rel_pos_attention_infer)
    monkeypatch.setattr(attention, "rel_pos_attention_infer", c)
    return c


@pytest.mark.parametrize("precision", [2, 32])
def test_logits_match_oracle_on_the_long_kernel(model, batch, gpu, infer_calls, precision):
    from oracle.conformer_oracle import OracleConformer

    orc = OracleConformer(model.state_dict(), **CFG_ORACLE)
    with torch.no_grad():
        _, mask_p, lg_p = model(_to(batch, gpu), precision)
        _, mask_o, lg_o = orc(batch, precision, None)
    assert infer_calls.n == N_BLOCKS
    assert mask_p.sum(1).tolist() == SUB_LENS
    assert torch.equal(mask_p.cpu(), mask_o)
    err = (lg_p.cpu() - lg_o).abs().max().item()
    print(f"precision {precision}: logits max|err| {err:.3e}")
    assert err <= 1e-3, err


@pytest.mark.parametrize("decoder", ["greedy", "beam"])
def test_decoders_run_on_the_long_batch(model, batch, gpu, infer_calls, decoder):
    from onebit_asr.infer import encode_and_decode

    out, cnt, logits = encode_and_decode(model, _to(batch, gpu), precision=2, decoder=decoder)
    assert infer_calls.n == N_BLOCKS
    assert torch.isfinite(logits).all()
    cnt = cnt.cpu().tolist()
    assert all(0 <= c <= n for c, n in zip(cnt, SUB_LENS)), cnt


def test_graphed_inference_matches_eager(model, batch, gpu):
    from onebit_asr.infer import GraphedInference, encode_and_decode

    b = _to(batch, gpu)
    gi = GraphedInference(model, precision=2, act_quant=None)
    gi.run(b)  # captures (the long kernel has no host synchronisation) and replays
    _, _, logits = gi.run(b)
    _, _, e_logits = encode_and_decode(model, b, precision=2)
    err = (logits - e_logits).abs().max().item()
    assert err <= 1e-4 * e_logits.abs().max().item(), err


def _forward(model, b, grad):
    with torch.enable_grad() if grad else torch.no_grad():
        return model(b, 2)[2].detach()


@pytest.mark.parametrize("case", ["grad", "train_dropout", "env_torch"])
def test_routing_negatives_take_the_torch_path(model, batch, gpu, infer_calls, monkeypatch, case):
    from onebit_asr import fused

    b = _to(batch, gpu)
    grad = case == "grad"
    if case == "train_dropout":
        model.train()
    try:
        runs = []
        snap = fused.rng_snapshot(gpu)
        for env in (case == "env_torch", True):  # as routed, then the torch path asked for by name
            if env:
                monkeypatch.setenv("OB_ATTN", "torch")
            torch.manual_seed(5)
            fused.rng_restore(gpu, snap)
            runs.append(_forward(model, b, grad))
    finally:
        model.eval()
    assert infer_calls.n == 0
    assert torch.equal(runs[0], runs[1])


def test_short_batch_keeps_the_fused_kernel(model, gpu, infer_calls, monkeypatch):
    from onebit_asr import conformer
    from onebit_asr.data import synthetic_batch

    fwd = Counter(conformer.rel_pos_attention)
    monkeypatch.setattr(conformer, "rel_pos_attention", fwd)
    b = synthetic_batch([2051, 900], [9, 9], vocab=VOCAB, seed=1, device=gpu)  # T' = 512
    with torch.no_grad():
        _, mask, _ = model(b, 2)
    assert mask.size(1) == 512
    assert infer_calls.n == 0 and fwd.n == N_BLOCKS


def test_int8_activation_model_routes_to_the_long_kernel(model, batch, gpu, infer_calls):
    from onebit_asr.quant import set_act_quant

    set_act_quant(model, "absmax_int8")
    try:
        with torch.no_grad():
            logits = model(_to(batch, gpu), 2)[2]
    finally:
        set_act_quant(model, None)
    assert infer_calls.n == N_BLOCKS
    assert torch.isfinite(logits).all()
