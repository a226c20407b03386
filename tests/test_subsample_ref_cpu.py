"""CPU: the float64 reference of the subsampling convolutions (tests/subsample_ref.py) is right,
the bars of tests/test_subsample_family_gpu.py leave float32 arithmetic a factor of two at
every row of its matrix, the exact-integer inputs are exact and have ReLU ties, `plan` gives
every row the launch property it is there for, and the C ABI rejects bad arguments before any
launch (nothing here touches a GPU)."""
import pytest
import torch

import subsample_ref as R

OB_ERR_NULL, OB_ERR_SHAPE, OB_ERR_WORKSPACE, OB_ERR_ALIGN = -1, -2, -4, -5


# ---------------------------------------------------------------------------------------
# (a) the reference against F.conv2d / relu autograd, float64


def _autograd(t):
    F = torch.nn.functional
    x, dy2 = t["x"].double(), t["dy2"].double()
    p = [t[k].double().clone().requires_grad_(True) for k in ("w0", "b0", "w2", "b2")]
    y1 = F.relu(F.conv2d(x[:, None], p[0], p[1], stride=2))
    y2 = F.relu(F.conv2d(y1, p[2], p[3], stride=2))
    (y2.permute(0, 2, 3, 1) * dy2).sum().backward()
    out = {"Y1": y1.detach().permute(0, 2, 3, 1), "Y2": y2.detach().permute(0, 2, 3, 1)}
    out.update(zip(R.GRADS, (q.grad for q in p)))
    return out


@pytest.mark.parametrize("F", [11, 12, 13, 14])
@pytest.mark.parametrize("T", [11, 12, 13, 14])
def test_reference_equals_conv2d_autograd(T, F):
    """Outputs and the four gradients to 1e-12 relative, at every residue of T and F mod 4
    (T1, F1 in {5, 6}, T2 = F2 = 2; the last row / column of X and of Y1 used or not)."""
    t = R.inputs(3, T, F, 48)
    ref, want = R.run(t), _autograd(t)
    for k in R.FWD + R.GRADS:
        assert ref[k].shape == want[k].shape, k
        err = (ref[k] - want[k]).abs().max().item()
        assert err <= 1e-12 * want[k].abs().max().item(), (k, err)
    # dY1 localises a failure: it is the gradient of the masked sum with respect to Y1
    y1 = ref["Y1"].clone().requires_grad_(True)
    pre2 = sum(torch.einsum("btfc,oc->btfo", R._win(y1, i, j, *ref["Y2"].shape[1:3]),
                            t["w2"].double()[:, :, i, j]) for i, j in R.TAPS) + t["b2"].double()
    (torch.relu(pre2) * t["dy2"].double()).sum().backward()
    assert (ref["dY1"] - y1.grad).abs().max().item() <= 1e-12 * y1.grad.abs().max().item()


def test_given_masks_replace_the_comparison():
    t = R.inputs(2, 11, 13, 48)
    ref = R.run(t)
    again = R.run(t, m1=ref["m1"], m2=ref["m2"])
    for k in R.FWD + R.GRADS:
        assert torch.equal(ref[k], again[k]), k
    none = R.run(t, m2=torch.zeros_like(ref["m2"]))
    assert (none["Y2"] == 0).all() and (none["dW2"] == 0).all() and (none["dW0"] == 0).all()
    assert torch.equal(none["Y1"], ref["Y1"])


# ---------------------------------------------------------------------------------------
# (b) float32 with the float64 masks stays below half of every bar, at every matrix row


def _marks(case):
    return [pytest.mark.slow] if case[0] == "shipped" else []


@pytest.mark.parametrize("case", [pytest.param(c, marks=_marks(c)) for c in R.CASES], ids=R.CASE_IDS)
def test_float32_alone_keeps_half_of_every_bar(case):
    """The bars are the project's 1e-5 forms. Plain float32 torch (the same tap loops and
    einsums, masks pinned to the float64 ones) is the yardstick for what the format costs: the
    worst err / bar over the matrix was 0.072 (dW0 max-form, (16, 1000, 80, 48); 0.054 below
    the shipped geometry) when this was written, so no bar is widened."""
    _, _, shape = case
    t = R.inputs(*shape)
    ref = R.run(t)
    got = R.run(t, torch.float32, m1=ref["m1"], m2=ref["m2"])
    for k in R.GRADS:
        assert ref[k].norm().item() > 0, f"{k}: an all-zero reference checks nothing"
    worst = {}
    for q, (err, bar) in R.errors(got, ref).items():
        worst[q] = err / bar
        assert err <= 0.5 * bar, f"{shape} {q}: float32 err {err:.3e} > half of the bar {bar:.3e}"
    print(f"\n{shape} float32 err/bar: " + "  ".join(f"{q} {v:.3f}" for q, v in worst.items()))


def test_one_mask_flip_is_visible_at_the_shipped_scale():
    """Why the masks are pinned, and what a wrong relu'(Y1) recompute would look like: flipping
    m1 in the one element with the largest |dY1 * X| moves dW0 by far more than its bar."""
    t = R.inputs(5, 301, 80, 48)
    ref = R.run(t)
    m1 = ref["m1"].clone()
    idx = (ref["dY1"].abs() * ref["m1"]).argmax().item()
    m1.view(-1)[idx] = False
    bad = R.run(t, m1=m1, m2=ref["m2"])
    e = R.errors(bad, ref, keys=("dW0", "db0"))
    assert e["db0/max"][0] > 10 * e["db0/max"][1], e


# ---------------------------------------------------------------------------------------
# (c) the exact-integer inputs


@pytest.mark.parametrize("shape", R.INT_CASES, ids=str)
def test_integer_inputs_are_exact_and_have_ties(shape):
    t = R.inputs(*shape, "int")
    ref = R.run(t, abs_sums=True)
    for k, v in t.items():
        assert torch.equal(v, v.round()) and v.abs().max() < 256, k
    nz = (t["w2"] != 0).float().mean().item()
    assert 0.08 < nz < 0.12, nz
    for k, v in ref["abs"].items():
        assert v < 2 ** 24, f"{k}: sum of absolute terms {v:.0f}"
    ties1 = int((ref["pre1"] == 0).sum())
    ties2 = int((ref["pre2"] == 0).sum())
    assert ties1 > 0 and ties2 > 0, (ties1, ties2)
    # a tie with a gradient behind it: `>=` in place of `>` would change db2 / db0
    assert ((ref["pre2"] == 0) & (t["dy2"] != 0)).any()
    assert ((ref["pre1"] == 0) & (ref["dY1"] != 0)).any()
    assert ref["Y1"].max() < 256 and t["dy2"].abs().max() < 256  # the bf16 hi plane holds the GEMM operands
    f32 = R.run(t, torch.float32)
    for k in R.FWD + R.GRADS:
        assert torch.equal(f32[k].double(), ref[k]), k
        assert ref[k].abs().max() > 0, k
    print(f"\n{shape} int: ties pre1 {ties1}/{ref['pre1'].numel()}  pre2 {ties2}/{ref['pre2'].numel()}"
          f"  max Y1 {ref['Y1'].max():.0f} Y2 {ref['Y2'].max():.0f}"
          f"  grads {max(ref[k].abs().max().item() for k in R.GRADS):.0f}  abs sums {ref['abs']}")


# ---------------------------------------------------------------------------------------
# (d) plan


@pytest.mark.parametrize("case", R.CASES, ids=R.CASE_IDS)
def test_plan_puts_each_row_in_its_class(case):
    R.check_plan(*case)


def test_plan_of_the_matrix_as_a_whole():
    rows = {name: R.plan(*shape) for _, name, shape in R.CASES}
    # the input parities: every combination of an unused last row / column of X and of Y1
    assert len({p["unused"] for n, p in rows.items() if n.startswith("parity") and "F80" not in n}) == 16
    assert len({p["unused"][:2] for n, p in rows.items() if n.endswith("F80")}) == 4
    # the finish kernel's 16 loads in flight: 15, 16 and 17 chunks, and one chunk
    assert {15, 16, 17, 1, 28} <= {p["wgrad"]["chunks"] for p in rows.values()}
    assert {1, 2, 3, 4, 5} <= {p["wgrad"]["steps_first"] for p in rows.values()}
    # only the shipped geometry loops over tiles; nothing smaller does (so the old file's
    # largest shape does not either)
    for name, p in rows.items():
        looped = p["fwd"]["tiles_per_block"][1] > 1
        assert looped == (name in ("C48", "C64", "C96", "C144")), name
    old = R.plan(5, 301, 80, 144)
    assert old["M"] == 7030 and old["fwd"]["tiles"] == 55 and old["fwd"]["tiles_per_block"] == (1, 1)
    assert all(c["tiles_per_block"][1] == 1 for c in old["dgrad"])
    assert old["conv0"]["passes"] == 1
    # the benchmark's shape
    b = R.plan(32, 1000, 80, 144)
    assert b["fwd"]["tiles_per_block"] == (2, 3) and b["conv0"]["passes"] == 11
    assert [c["tiles_per_block"] for c in b["dgrad"]] == [(6, 7), (10, 11), (10, 11), (15, 16)]
    assert sum(c["nblk"] for c in b["dgrad"]) <= R.DGRAD_BLOCKS


def test_plan_workspace_matches_the_library():
    """The one number of the launch arithmetic the ABI shows: the workspace holds G, `chunks`
    partial dW2 / db2 slabs and 508 conv0 partials, each rounded up to 256 bytes."""
    from onebit_asr import _lib

    lib = _lib.load()
    up = lambda n: (n + 255) & ~255  # noqa: E731
    for _, _, (B, T, F, C) in R.CASES:
        p = R.plan(B, T, F, C)
        want = (up(p["M"] * C * 4) + up(p["wgrad"]["chunks"] * C * 9 * C * 4)
                + up(p["wgrad"]["chunks"] * C * 4) + up(R.DGRAD_BLOCKS * C * 10 * 4))
        assert lib.ob_subsample_bwd_workspace(B, T, F, C) == want, (B, T, F, C)
        assert p["dgrad_blocks"] <= R.DGRAD_BLOCKS


# ---------------------------------------------------------------------------------------
# (e) argument rejection, before any launch


def test_argument_rejection_without_gpu():
    """Every call below returns from capi.hip's checks (shape, then null, then workspace, then
    alignment) before a HIP call; the pointers are never dereferenced."""
    from onebit_asr import _lib

    lib = _lib.load()
    fake = 0x1000  # 16-byte aligned

    def fwd(B=2, T=20, F=20, C=48, X=fake, Y1=fake, img=fake):
        return lib.ob_subsample_fwd(X, B, T, F, C, fake, fake, img, fake, Y1, fake, None)

    def bwd(B=2, T=20, F=20, C=48, X=fake, Y1=fake, ws=fake, wsb=None, dW0=fake):
        wsb = lib.ob_subsample_bwd_workspace(B, T, F, C) if wsb is None else wsb
        return lib.ob_subsample_bwd(X, fake, fake, Y1, fake, fake, B, T, F, C, fake, dW0, fake, fake,
                                    fake, ws, wsb, None)

    assert lib.ob_subsample_bwd_workspace(2, 20, 20, 48) > 0
    big = dict(B=4096, T=1000, F=80, C=144)  # B * T1 * F1 * C = 2^12 * 499 * 39 * 144 >= 2^30
    assert 4096 * 499 * 39 * 144 >= 2 ** 30
    for bad in (dict(C=32), dict(C=80), dict(C=160), dict(T=6), dict(F=6), dict(B=0), dict(B=65536), big):
        assert fwd(**bad) == OB_ERR_SHAPE, bad
        assert bwd(wsb=1 << 40, **bad) == OB_ERR_SHAPE, bad
        args = dict(dict(B=2, T=20, F=20, C=48), **bad)
        assert lib.ob_subsample_bwd_workspace(args["B"], args["T"], args["F"], args["C"]) == 0, bad
    for C in (32, 80, 160):
        assert lib.ob_subsample_image_bytes(C) == 0
        assert lib.ob_subsample_pack(fake, C, fake, None) == OB_ERR_SHAPE
    # the largest batch the ABI takes is a shape it accepts (and then a null pointer stops it)
    assert fwd(B=65535, T=7, F=7, X=None) == OB_ERR_NULL
    assert fwd(X=None) == OB_ERR_NULL and fwd(Y1=None) == OB_ERR_NULL and fwd(img=None) == OB_ERR_NULL
    assert bwd(X=None) == OB_ERR_NULL and bwd(ws=None) == OB_ERR_NULL and bwd(dW0=None) == OB_ERR_NULL
    assert lib.ob_subsample_pack(None, 48, fake, None) == OB_ERR_NULL
    assert fwd(Y1=fake + 4) == OB_ERR_ALIGN and fwd(X=fake + 2) == OB_ERR_ALIGN
    assert bwd(Y1=fake + 4) == OB_ERR_ALIGN and bwd(ws=fake + 8) == OB_ERR_ALIGN
    assert lib.ob_subsample_pack(fake, 48, fake + 8, None) == OB_ERR_ALIGN
    need = lib.ob_subsample_bwd_workspace(2, 20, 20, 48)
    assert bwd(wsb=need - 1) == OB_ERR_WORKSPACE
    assert bwd(wsb=need - 1, Y1=fake + 4) == OB_ERR_WORKSPACE  # the size is checked first
    for C in R.CS:
        assert lib.ob_subsample_image_bytes(C) > 0 and lib.ob_subsample_image_bytes(C) % 16 == 0
