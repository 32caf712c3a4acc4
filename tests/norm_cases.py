"""Inputs away from N(0,1) for the normalisation and softmax kernels, with their float64 and fp32-CPU references.

Plain functions, seeded torch.Generators, no GPU: tests/test_norm_offset_cpu.py proves on the CPU that every case is FAIR (the
reference's own fp32 arithmetic stays within E_REF_MAX of float64 on it) and tests/test_norm_offset_gpu.py holds the HIP kernels to
`bar(E_ref)` on the identical tensors.  One metric throughout: E = max-abs against the float64 result, E_ref = the same for the
fp32 CPU reference.  Every function returns the same bits on every call; cached results are shared and must not be written to.
"""
import functools
import zlib

import torch
import torch.nn.functional as F

E_REF_MAX = 5e-5          # the fairness condition: a case whose fp32 reference misses it is redrawn or dropped, on the CPU


def bar(e_ref):
    """4 E_ref + 2e-6.  2x: the library's folded x*A + B rounds B at |mean| rstd where torch rounds (x - mean) once; 2x: another summation
    order; the floor is a tenth of the suite's standing 2e-5 single-op bound (the noise of the centred cases)."""
    return 4.0 * e_ref + 2e-6


def err(got, want):
    return float((got.double() - want.double()).abs().max())


def rel_err(got, want):
    return err(got, want) / max(1e-6, float(want.double().abs().max()))


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


# ---- GroupNorm32 / LayerNorm inputs -------------------------------------------------------------------------------------------------
OFFSETS = (0, 3, 10, 30, 100)
GN_FLAVOURS = tuple(f"offset{r}" for r in OFFSETS) + ("channel_offsets", "constant_group", "tiny_variance", "mixed")
_MIXED = ("offset100", "tiny_variance", "constant_group", "channel_offsets", "offset30", "offset0")   # image i of `mixed` takes entry i mod 6

# the shapes of the GPU tests, by the statistics kernel they reach (N, C, H, W)
GN_SMALL_SHAPES = [(2, 128, 8, 8),       # k_gn_small<4>
                   (2, 64, 8, 8),        # <2>
                   (2, 96, 5, 7),        # <1>, 3 channels per group, odd slab
                   (2, 32, 8, 8)]        # <1>, one channel per group
GN_CHUNKED_SHAPES = [(1, 64, 96, 96),    # k_gn_partial + k_gn_coef: 36 chunks
                     (1, 96, 80, 72),    # 22 chunks, ragged last chunk, float4 columns that straddle groups
                     (2, 192, 64, 64)]   # 16 chunks, two images
GN_TRAIN_SHAPES = [(2, 64, 8, 8), (1, 96, 80, 72)]
LN_SHAPES = [(37, 20), (128, 256), (512, 128)]


def gn_input(flavour, shape):
    """(N,C,H,W) fp32.  offset<r>: randn + r; channel_offsets: randn + 10 randn(1,C,1,1) (between-channel spread dominates a group's
    variance); constant_group: group 0 of every image is exactly 0.1 (variance 0, rstd = eps^-1/2), the rest randn; tiny_variance:
    1e-3 randn + 0.01 (eps dominates); mixed: another flavour per image."""
    N, C, H, W = shape
    g = _gen("gn", flavour, shape)
    if flavour == "mixed":
        return torch.cat([gn_input(_MIXED[i % len(_MIXED)], (1, C, H, W)) for i in range(N)], 0)
    x = torch.randn(shape, generator=g)
    if flavour.startswith("offset"):
        return x + float(flavour[6:])
    if flavour == "channel_offsets":
        return x + 10.0 * torch.randn((1, C, 1, 1), generator=g)
    if flavour == "constant_group":
        x[:, :C // 32] = 0.1
        return x
    if flavour == "tiny_variance":
        return 1e-3 * x + 0.01
    raise KeyError(flavour)


def gn_params(shape):
    """gamma, beta (C) and the scale/shift rows (N, 2C) as the suite's other GroupNorm tests draw them."""
    N, C = shape[:2]
    g = _gen("gn_params", shape)
    return torch.randn(C, generator=g) * 0.2 + 1, torch.randn(C, generator=g) * 0.2, torch.randn((N, 2 * C), generator=g) * 0.3


def gn_forward(x, gamma, beta, emb, eps, silu=False):
    """silu?( GroupNorm32(x) [* (1 + scale) + shift] ) in the dtype of x (nn.py:17-19,100; unet.py:203-206)."""
    C = x.shape[1]
    u = F.group_norm(x, 32, gamma, beta, eps)
    if emb is not None:
        u = u * (1 + emb[:, :C, None, None]) + emb[:, C:, None, None]
    return u * torch.sigmoid(u) if silu else u


def gn_stats64(x):
    """float64 group statistics: mean and biased variance, (N, 32) each."""
    xd = x.double().reshape(x.shape[0], 32, -1)
    return xd.mean(2), xd.var(2, unbiased=False)


def gn_ratio(x):
    """largest |mean| / std over the (image, group)s with a variance (what the case achieves)."""
    m, v = gn_stats64(x)
    ok = v > 0
    return float((m.abs()[ok] / v[ok].sqrt()).max()) if bool(ok.any()) else 0.0


@functools.lru_cache(maxsize=None)
def gn_case(flavour, shape, use_emb, eps=1e-5):
    """The case with both references: x, gamma, beta, emb, want (float64), ref32 (F.group_norm on the CPU), e_ref, and for the statistics
    stat64 = (mean, rstd) in float64 next to stat32 = torch.native_group_norm's fp32 pair."""
    x = gn_input(flavour, shape)
    gamma, beta, emb = gn_params(shape)
    emb = emb if use_emb else None
    d = lambda t: None if t is None else t.double()  # noqa: E731
    want = gn_forward(x.double(), d(gamma), d(beta), d(emb), eps)
    ref32 = gn_forward(x, gamma, beta, emb, eps)
    N, C, H, W = shape
    _, m32, r32 = torch.native_group_norm(x, gamma, beta, N, C, H * W, 32, eps)
    m64, v64 = gn_stats64(x)
    return dict(x=x, gamma=gamma, beta=beta, emb=emb, want=want, ref32=ref32, e_ref=err(ref32, want), stat64=(m64, 1.0 / torch.sqrt(v64 + eps)),
                stat32=(m32.reshape(N, 32), r32.reshape(N, 32)))


def ln_input(r, shape):
    return torch.randn(shape, generator=_gen("ln", r, shape)) + float(r)


@functools.lru_cache(maxsize=None)
def ln_case(r, shape, eps=1e-5):
    P, C = shape
    x = ln_input(r, shape)
    g = _gen("ln_params", shape)
    gamma, beta = torch.randn(C, generator=g) * 0.2 + 1, torch.randn(C, generator=g) * 0.2
    cot = torch.randn(shape, generator=g)
    want = F.layer_norm(x.double(), (C,), gamma.double(), beta.double(), eps)
    ref32 = F.layer_norm(x, (C,), gamma, beta, eps)
    return dict(x=x, gamma=gamma, beta=beta, cot=cot, want=want, ref32=ref32, e_ref=err(ref32, want))


# ---- attention inputs ----------------------------------------------------------------------------------------------------------------
ATTN_FLAVOURS = ("plain", "logit_offset+100", "logit_offset-100", "peaked", "one_hot")
# (N, T, C, heads) by forward kernel
ATTN_SHAPES = [(1, 33, 128, 4),      # k_attention<32>, a ragged second row / key tile
               (1, 1, 128, 4),       # one token
               (1, 40, 256, 4),      # k_attention<64>
               (1, 40, 512, 4),      # k_attention<128>
               (1, 100, 384, 4),     # k_attention_ks<96>: four key tiles, the last with 4 valid keys
               (1, 64, 768, 4),      # k_attention_ks<192>: two key tiles, two of the four key-split waves idle
               (1, 40, 64, 4)]       # k_attention_generic, head size 16
ATTN_BWD_SHAPES = [(2, 40, 128, 4), (1, 100, 384, 4), (1, 64, 768, 4), (2, 40, 64, 4)]


def attention(qkv, heads):
    """QKVAttention (unet.py:255-274) on (N, 3C, T) in the dtype of qkv, as test_attention_matches_torch writes it -> (N, C, T)."""
    N, C3, T = qkv.shape
    ch = C3 // 3 // heads
    q, k, v = qkv.reshape(N * heads, 3 * ch, T).split(ch, dim=1)
    s = 1.0 / (ch ** 0.25)
    wgt = torch.softmax(torch.einsum("bct,bcs->bts", q * s, k * s), dim=-1)
    return torch.einsum("bts,bcs->bct", wgt, v).reshape(N, C3 // 3, T)


def _top_probability(qkv, heads):
    """float64 softmax rows of the case: (largest probability per row, its key, the smallest lead of a row's top score over its second)."""
    N, C3, T = qkv.shape
    ch = C3 // 3 // heads
    q, k, _ = qkv.double().reshape(N * heads, 3 * ch, T).split(ch, dim=1)
    sc = torch.einsum("bct,bcs->bts", q, k) / ch ** 0.5
    top, key = torch.softmax(sc, dim=-1).max(dim=-1)
    two = sc.topk(min(2, T), dim=-1).values
    return top, key, float((two[..., 0] - two[..., -1]).min()) if T > 1 else float("inf")


def attn_qkv(flavour, shape):
    """(N, 3C, T) fp32, the reference's layout (head-major [q|k|v] blocks of ch channels).

    plain: unit Gaussian.  logit_offset<d> (d = +100, -100, or 0 for the baseline the other two must reproduce): the plain draw with
    channel 0 of every head's q set to (|d| sqrt(ch))^1/2 and of its k to +-that for every token, so every score moves by d and the
    softmax is mathematically unchanged.  peaked: q rows of norm sqrt(ch), k_j = gain q_(T-1-j) with the gain searched so that every
    row's top probability lies in [0.5, 0.999] (asserted in float64): the first queries' winning key sits in the last key tile.
    one_hot: the same with a gain that leaves every other key at least e^-40 behind (asserted)."""
    N, T, C, heads = shape
    ch = C // heads
    x = torch.randn((N * heads, 3, ch, T), generator=_gen("attn", shape))
    if flavour.startswith("logit_offset"):
        d = float(flavour[len("logit_offset"):])
        a = (abs(d) * ch ** 0.5) ** 0.5
        x[:, 0, 0, :] = a
        x[:, 1, 0, :] = a if d >= 0 else -a
    elif flavour in ("peaked", "one_hot"):
        q = x[:, 0]
        q = q * (ch ** 0.5 / q.double().norm(dim=1, keepdim=True)).float()
        x[:, 0] = q
        want_key = torch.arange(T - 1, -1, -1).expand(N * heads, T)
        gain, found = 0.125, False
        while gain < 4096 and not found:
            gain *= 1.0625 if flavour == "peaked" else 2.0
            x[:, 1] = gain * q.flip(-1)
            top, key, lead = _top_probability(x.reshape(N, 3 * C, T), heads)
            if flavour == "peaked":
                found = T == 1 or (float(top.min()) >= 0.5 and float(top.max()) <= 0.999)
            else:
                found = lead >= 40.0        # every other key at most e^-40 of the winner: the top probability is 1 in fp32 and in float64
        assert found, (flavour, shape)
        assert torch.equal(key, want_key), (flavour, shape)
    elif flavour != "plain":
        raise KeyError(flavour)
    return x.reshape(N, 3 * C, T)


@functools.lru_cache(maxsize=None)
def attn_case(flavour, shape):
    qkv = attn_qkv(flavour, shape)
    heads = shape[3]
    want = attention(qkv.double(), heads)
    ref32 = attention(qkv, heads)
    return dict(qkv=qkv, want=want, ref32=ref32, e_ref=err(ref32, want))


# ---- whole networks with GroupNorm inputs away from zero -------------------------------------------------------------------------------
NET_KINDS = ("controlnet", "xattn")
# bias shift -> the 90th percentile of mean / std over every (GroupNorm input, image, group): 3.0 -> ~10, 10.0 -> ~30 (the largest: ~30 and ~110).
# The residual streams carry the shift on with a spread of their own, so the median stays near 3 whatever the shift.
NET_SHIFTS = (3.0, 10.0)


def _net_model(kind):
    from humanliff_amd import synthetic as syn
    from humanliff_amd.improved_diffusion.script_util import create_model_and_diffusion, model_and_diffusion_defaults
    a = model_and_diffusion_defaults()
    if kind == "controlnet":            # the tiny model of tests/test_train_loss_cpu.py
        a.update(dict(in_channels=27, out_channels=27, class_cond=True, learn_sigma=False, num_heads=4, use_scale_shift_norm=True, cond_type="controlnet",
                      rescale_timesteps=False, dropout=0.0, image_size=32, num_channels=32, num_res_blocks=1, attention_resolutions="16,8"))
        size = 16
    else:                               # the cross-attention model of tests/train_variants_cases.py: its context Linear fixes x_cond at 256 x 256
        from tests import train_variants_cases as tv
        a.update(tv.case_overrides("xattn"))
        size = 256
    model, _ = create_model_and_diffusion(**a)
    model.load_state_dict(syn.state_from_shapes([(k, tuple(v.shape)) for k, v in model.state_dict().items()], 1), strict=True)
    g = _gen("net", kind)
    x = torch.randn((2, 27, size, size), generator=g)
    xc = torch.randn((2, 27, size, size), generator=g).clamp(-1, 1) * 0.7
    return model.eval(), (x, torch.tensor([999, 17]), xc, torch.tensor([3, 0]))


def net_shift_biases(model, shift):
    """Adds `shift` to the bias of every convolution whose output a GroupNorm reads directly or through a residual sum: the first convolution
    of each encoder, both 3x3 convolutions of every ResBlock, the Downsample / Upsample convolutions.  Returns how many."""
    from humanliff_amd.improved_diffusion import unet as U
    convs = [m.in_layers[2] for m in model.modules() if isinstance(m, U.ResBlock)] + [m.out_layers[3] for m in model.modules() if isinstance(m, U.ResBlock)]
    convs += [m.op for m in model.modules() if isinstance(m, U.Downsample)] + [m.conv for m in model.modules() if isinstance(m, U.Upsample)]
    convs += [model.input_blocks[0][0]] + ([model.input_blocks_cond[0][0]] if getattr(model, "cond_type", "") == "controlnet" else [])
    with torch.no_grad():
        for c in convs:
            c.bias += shift
    return len(convs)


@functools.lru_cache(maxsize=None)
def net_case(kind, shift):
    """model (fp32, CPU, biases shifted), args = (x, t, x_cond, y), want (float64 twin), ref32 (fp32 twin), e_ref relative to max(1, |out|max),
    ratios = |mean| / std of every (GroupNorm input, image, group) the fp32 twin saw."""
    import copy
    from unittest import mock
    from tests.unet_autograd_twin import forward_autograd
    model, (x, t, xc, y) = _net_model(kind)
    net_shift_biases(model, shift)
    ratios = []
    real = F.group_norm

    def recording(inp, groups, *a, **k):
        m, v = inp.double().reshape(inp.shape[0], groups, -1).mean(2), inp.double().reshape(inp.shape[0], groups, -1).var(2, unbiased=False)
        ratios.append((m.abs() / v.clamp_min(1e-30).sqrt()).flatten())
        return real(inp, groups, *a, **k)

    with torch.no_grad():
        with mock.patch.object(F, "group_norm", recording):
            ref32 = forward_autograd(model, x, t, xc, y=y)
        want = forward_autograd(copy.deepcopy(model).double(), x.double(), t, xc.double(), y=y)
    scale = max(1.0, float(want.abs().max()))
    return dict(model=model, args=(x, t, xc, y), want=want, ref32=ref32, scale=scale, e_ref=err(ref32, want) / scale, ratios=torch.cat(ratios))
