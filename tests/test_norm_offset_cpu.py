"""The cases of tests/norm_cases.py are fair and deterministic (no GPU): on every tensor the GPU tests use, the reference's own fp32
arithmetic on the CPU - F.group_norm, torch.native_group_norm's (mean, rstd), F.layer_norm, the QKVAttention einsums - stays within
E_REF_MAX = 5e-5 (max-abs) of float64.  tests/test_norm_offset_gpu.py holds the HIP kernels to 4 E_ref + 2e-6 on the same tensors; a
case that misses the condition here is redrawn or dropped here, never loosened there."""
import pytest
import torch

from tests import norm_cases as nc

GN_SHAPES = nc.GN_SMALL_SHAPES + nc.GN_CHUNKED_SHAPES


@pytest.mark.parametrize("shape", GN_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("flavour", nc.GN_FLAVOURS)
def test_groupnorm_cases_are_fair(flavour, shape):
    N = shape[0]
    for use_emb in (False, True):
        c = nc.gn_case(flavour, shape, use_emb)
        (m64, r64), (m32, r32) = c["stat64"], c["stat32"]
        e_mean = float(((m32.double() - m64).abs() * r64).max())          # in units of the group's std: what it does to the output
        e_rstd = float(((r32.double() - r64).abs() / r64).max())
        print(f"GroupNorm {flavour} {shape} emb={use_emb}: mean/std {nc.gn_ratio(c['x']):.1f}  E_ref {c['e_ref']:.2e}  "
              f"native mean {e_mean:.2e} (std)  rstd {e_rstd:.2e} (rel)")
        assert c["e_ref"] <= nc.E_REF_MAX
        assert e_mean <= nc.E_REF_MAX and e_rstd <= nc.E_REF_MAX
    x = nc.gn_input(flavour, shape)
    if flavour.startswith("offset"):
        r = float(flavour[6:])
        assert abs(float(x.double().mean()) - r) < 0.05 and abs(float(x.double().std()) - 1) < 0.05
    if flavour == "constant_group":
        grp = x.reshape(N, 32, -1)[:, 0]
        assert torch.equal(grp, torch.full_like(grp, 0.1))
        assert float(nc.gn_case(flavour, shape, False)["stat64"][1][:, 0].min()) == pytest.approx(1e-5 ** -0.5)
    assert torch.equal(x, nc.gn_input(flavour, shape))                   # two calls, the same bits


@pytest.mark.parametrize("shape", GN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_groupnorm_training_cases_are_fair_at_eps_1e6(shape):
    """The SpatialTransformer's norm (eps 1e-6) on the same tensors."""
    for flavour in nc.GN_FLAVOURS:
        c = nc.gn_case(flavour, shape, False, 1e-6)
        print(f"GroupNorm eps 1e-6 {flavour} {shape}: E_ref {c['e_ref']:.2e}")
        assert c["e_ref"] <= nc.E_REF_MAX


@pytest.mark.parametrize("shape", nc.LN_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("r", nc.OFFSETS)
def test_layernorm_cases_are_fair(r, shape):
    c = nc.ln_case(r, shape)
    print(f"LayerNorm offset{r} {shape}: E_ref {c['e_ref']:.2e}")
    assert c["e_ref"] <= nc.E_REF_MAX
    assert torch.equal(c["x"], nc.ln_input(r, shape))


@pytest.mark.parametrize("shape", list(dict.fromkeys(nc.ATTN_SHAPES + nc.ATTN_BWD_SHAPES)), ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("flavour", nc.ATTN_FLAVOURS + ("logit_offset0",))
def test_attention_cases_are_fair(flavour, shape):
    N, T, C, heads = shape
    c = nc.attn_case(flavour, shape)
    top, key, lead = nc._top_probability(c["qkv"], heads)
    print(f"attention {flavour} {shape}: E_ref {c['e_ref']:.2e}  top probability {float(top.min()):.3f} .. {float(top.max()):.3f}  lead {lead:.1f}")
    assert c["e_ref"] <= nc.E_REF_MAX
    assert torch.equal(c["qkv"], nc.attn_qkv(flavour, shape))
    ch = C // heads
    if flavour.startswith("logit_offset"):
        # every score moved by the same amount: the float64 softmax output is the baseline's (the channel set to zero)
        d = float(flavour[len("logit_offset"):])
        q, k, _ = c["qkv"].double().reshape(N * heads, 3 * ch, T).split(ch, dim=1)
        assert float((q[:, 0] * k[:, 0] / ch ** 0.5 - d).abs().max()) < 1e-4
        base = nc.attn_case("logit_offset0", shape)
        assert nc.err(c["want"], base["want"]) < 1e-12
    if flavour == "peaked" and T > 1:
        assert 0.5 <= float(top.min()) and float(top.max()) <= 0.999
        assert torch.equal(key, torch.arange(T - 1, -1, -1).expand(N * heads, T))    # the first queries win in the last key tile
    if flavour == "one_hot":
        assert float(top.min()) == 1.0 or T == 1
        _, _, v = c["qkv"].double().reshape(N * heads, 3 * ch, T).split(ch, dim=1)
        assert nc.err(c["want"], v.flip(-1).reshape(N, C, T)) < 1e-12             # the output IS the selected v row


@pytest.mark.parametrize("shift", nc.NET_SHIFTS)
@pytest.mark.parametrize("kind", nc.NET_KINDS)
def test_network_cases_are_fair(kind, shift):
    """Whole networks whose GroupNorm inputs sit away from zero: the fp32 twin stays within 1e-4 (relative to max(1, |out|max)) of the float64 twin."""
    c = nc.net_case(kind, shift)
    r = c["ratios"]
    print(f"network {kind} bias shift {shift}: GroupNorm input mean/std median {float(r.median()):.1f}  90% {float(r.quantile(0.9)):.1f}  "
          f"max {float(r.max()):.1f}  E_ref {c['e_ref']:.2e} (rel, |out|max {c['scale']:.2f})")
    assert c["e_ref"] <= 1e-4
    assert float(r.quantile(0.9)) >= 2.5 * shift          # the shift arrives where the norms read
    assert c["want"].dtype == torch.float64 and c["ref32"].dtype == torch.float32
