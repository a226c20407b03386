"""CPU checks of tests/convmod_ref.py, the float64 reference of the conv module core, and of
the inputs that tests/test_convmod_core_gpu.py feeds the kernels. No GPU, no product code.

1. `core` against an independent restatement with torch's own operators (per pass: F.glu ->
   F.conv1d(groups=C) -> F.batch_norm(training=True) -> y * sigmoid(y)) in float64: forward
   and every gradient to 1e-12 of the quantity's largest value. db_dw (and dw_dw at K = 1) are
   true zeros, sums of terms that cancel; their scale is the per-channel sum of |terms|.
2. Conditioning of every case of the GPU matrix and of the variants: `core` in float32 on the
   CPU against float64. The float32 error of each quantity must stay within a quarter of the
   GPU test's bar, so that a kernel exceeding a bar is wrong, not unlucky. A case that fails
   here is ill-conditioned and gets other inputs; the bars stay. (The bars against the
   statistics of the device's own z have no CPU counterpart: they check a reduction of given
   numbers.) The figures are printed at the end of the module.
3. One row per pass: the reference gives du, dw_dw and dgamma exactly 0 and v = swish(beta).
4. K = 1: the reference's dw_dw is zero to round-off (BatchNorm cancels a per-channel scale).
"""
import pytest
import torch
import torch.nn.functional as F

import convmod_ref as R

_ALL = R.CASES
_IDS = R.CASE_IDS
_VARIANTS = [(row, v) for row in R.VARIANT_ROWS for v in ("awkward", "saturated")]
_WORST = {}  # quantity -> (err / bar, err, bar, where)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if _WORST:
        print("\nfloat32 `core` on the CPU vs float64, worst case per quantity (err, bar, err/bar, where):")
        for q, (ratio, err, bar, where) in sorted(_WORST.items()):
            print(f"  {q:7s} {err:.3e}  bar {bar:.3e}  {ratio:.3f}  {where}")


def restated(t, dtype=torch.float64):
    """The same computation through torch's own GLU / conv1d / batch_norm, one pass at a time."""
    P, B, T, C, K, eps = t["P"], t["B"], t["T"], t["C"], t["K"], t["eps"]
    leaf = {k: t[k].to(dtype).clone().requires_grad_(True) for k in ("u", "w", "b", "gamma", "beta")}
    vs = []
    for p in range(P):
        x = leaf["u"][p * B * T:(p + 1) * B * T].view(B, T, 2 * C).transpose(1, 2)
        y = F.glu(x, dim=1)
        y = F.conv1d(y, leaf["w"].view(C, 1, K), leaf["b"], padding=K // 2, groups=C)
        y = F.batch_norm(y, None, None, leaf["gamma"], leaf["beta"], training=True, eps=eps)
        y = y * torch.sigmoid(y)
        vs.append(y.transpose(1, 2).reshape(B * T, C))
    v = torch.cat(vs)
    (v * t["dv"].to(dtype)).sum().backward()
    return {"v": v.detach(), "du": leaf["u"].grad, "dw_dw": leaf["w"].grad, "db_dw": leaf["b"].grad,
            "dgamma": leaf["gamma"].grad, "dbeta": leaf["beta"].grad}


@pytest.mark.parametrize("case", _ALL, ids=_IDS)
def test_core_equals_torch_operator_restatement(case):
    shape = case[2]
    t, ref = R.inputs(*shape), R.reference(*shape)
    alt = restated(t)
    K = shape[4]
    for q, a in alt.items():
        if q == "db_dw" or (q == "dw_dw" and K == 1):  # true zeros: the scale of what cancels
            terms = ref["dz"] if q == "db_dw" else ref["dz"] * ref["g"]
            scale = terms.abs().sum(dim=0).max().item()
        else:
            scale = ref[q].abs().max().item()
        err = (a - ref[q]).abs().max().item()
        assert err <= 1e-12 * scale, f"{q} {shape}: max|diff| {err:.3e} > 1e-12 * {scale:.3e}"


def _conditioned(shape, variant):
    t, ref = R.inputs(*shape, variant), R.reference(*shape, variant)
    got = R.run(t, torch.float32)
    bad = []
    for q, (err, bar) in R.errors(got, ref).items():
        ratio = err / bar
        where = f"{shape} {variant}"
        if q not in _WORST or ratio > _WORST[q][0]:
            _WORST[q] = (ratio, err, bar, where)
        if not err <= 0.25 * bar:
            bad.append(f"{q}: float32 err {err:.3e} > bar {bar:.3e} / 4")
    assert not bad, f"{shape} {variant} is ill-conditioned: " + "; ".join(bad)


@pytest.mark.parametrize("case", _ALL, ids=_IDS)
def test_matrix_case_is_well_conditioned(case):
    assert case[2][1] * case[2][2] >= 64, "fewer than 64 rows per pass"
    _conditioned(case[2], "std")


@pytest.mark.parametrize("case,variant", _VARIANTS, ids=[f"{c[0]}-{v}" for c, v in _VARIANTS])
def test_variant_is_well_conditioned(case, variant):
    _conditioned(case[2], variant)


@pytest.mark.parametrize("case", R.ONE_ROW, ids=[c[0] for c in R.ONE_ROW])
def test_one_row_per_pass_is_exact(case):
    shape = case[2]
    t, ref = R.inputs(*shape), R.reference(*shape)
    for q in ("du", "dw_dw", "dgamma"):
        assert (ref[q] == 0).all(), f"{q}: max|ref| {ref[q].abs().max().item():.3e}, expected exact zeros"
    beta = t["beta"].double()
    assert torch.equal(ref["v"], (beta * torch.sigmoid(beta)).expand(shape[0], -1))
    assert torch.allclose(ref["rstd"], torch.full_like(ref["rstd"], t["eps"] ** -0.5), rtol=1e-15)
    assert ref["dbeta"].abs().max() > 0
    # the float32 run is exact in the same places
    got = R.run(t, torch.float32)
    for q in ("du", "dw_dw", "dgamma"):
        assert (got[q] == 0).all(), q


def test_k1_weight_gradient_is_a_true_zero():
    shape = next(c[2] for c in R.CASES if c[2][4] == 1)
    ref = R.reference(*shape)
    terms = (ref["dz"] * ref["g"]).abs().sum(dim=0)
    ratio = (ref["dw_dw"].view(-1).abs() / terms).max().item()
    assert ratio <= 1e-9, f"max_c |dw_dw| / sum|dz * g| = {ratio:.3e}"
    # ... and so is the bias gradient, at every K
    for case in R.CASES[:3]:
        r = R.reference(*case[2])
        ratio = (r["db_dw"].abs() / r["dz"].abs().sum(dim=0)).max().item()
        assert ratio <= 1e-9, (case[2], ratio)


def test_awkward_variant_constant_channel():
    """The zero-weight channel: z is the bias, variance exactly 0, xhat exactly 0, rstd =
    1/sqrt(eps), and (xhat = 0) dgamma of that channel exactly 0 -- in float64 and float32."""
    for case in R.VARIANT_ROWS:
        shape = case[2]
        t = R.inputs(*shape, "awkward")
        c = t["info"]["const"]
        for dtype in (torch.float64, torch.float32):
            r = R.run(t, dtype)
            assert (r["z"][:, c] == t["b"][c].to(dtype)).all()
            assert (r["mean"][:, c] == t["b"][c].to(dtype)).all()
            assert (r["dgamma"][c] == 0).all()
            assert (r["du"][:, c] == 0).all() and (r["du"][:, shape[3] + c] == 0).all()
        ref = R.reference(*shape, "awkward")
        assert torch.allclose(ref["rstd"][:, c], torch.tensor(t["eps"] ** -0.5, dtype=torch.float64), rtol=1e-15)
