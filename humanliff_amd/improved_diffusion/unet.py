"""UNetModel with the reference's constructor, forward signature and state_dict layout
(human_diffusion/improved_diffusion/unet.py:323-615), executed by libhumanliff_hip.so.

The torch modules declared here only own the parameters (so reference checkpoints load with
load_state_dict and .to(device) works).  forward() hands the parameter pointers to the C ABI
(hl_unet_create / hl_unet_forward); there is no PyTorch implementation of the math and no CPU path.
Supported configuration: dims=2, use_scale_shift_norm True / False, cond_type in {"controlnet", "AdaGN", "cross_attention", "concat", ""},
use_3d_aware False or True (not with AdaGN / cross_attention).  Under no_grad / eval() forward() is the fused inference path; with gradients enabled on a model in training
mode it is the differentiable path of unet_train.py (HIP forward and backward kernels behind autograd.Functions), for every one of these
configurations (the 3-D-aware ResBlock needs use_scale_shift_norm=True, as in the reference).
"""
import ctypes as C

import torch as th
import torch.nn as nn

from .. import _lib
from .nn import SiLU, conv_nd, linear, normalization, zero_module


class TimestepBlock(nn.Module):
    pass


class TimestepEmbedSequential(nn.Sequential, TimestepBlock):
    pass


class Upsample(nn.Module):
    def __init__(self, channels, use_conv, dims=2):
        super().__init__()
        assert use_conv, "conv_resample=False is not built"
        self.channels, self.use_conv, self.dims = channels, use_conv, dims
        self.conv = conv_nd(dims, channels, channels, 3, padding=1)


class Downsample(nn.Module):
    def __init__(self, channels, use_conv, dims=2):
        super().__init__()
        assert use_conv, "conv_resample=False is not built"
        self.channels, self.use_conv, self.dims = channels, use_conv, dims
        self.op = conv_nd(dims, channels, channels, 3, stride=2, padding=1)


class ResBlock(TimestepBlock):
    def __init__(self, channels, emb_channels, dropout, out_channels=None, use_conv=False, use_scale_shift_norm=False,
                 use_3d_aware=False, dims=2, use_checkpoint=False):
        super().__init__()
        oc = out_channels or channels
        self.channels, self.emb_channels, self.dropout, self.out_channels = channels, emb_channels, dropout, oc
        self.use_3d_aware, self.use_scale_shift_norm = use_3d_aware, use_scale_shift_norm
        self.in_layers = nn.Sequential(normalization(channels), SiLU(), conv_nd(dims, channels, oc, 3, padding=1))
        self.emb_layers = nn.Sequential(SiLU(), linear(emb_channels, 2 * oc if use_scale_shift_norm else oc))      # unet.py:186-191
        # use_3d_aware (unet.py:158-166): the conv reads cat[h, two plane means of h] = 3*oc channels
        self.out_layers = nn.Sequential(normalization(oc), SiLU(), nn.Dropout(p=dropout),
                                        zero_module(conv_nd(dims, 3 * oc if use_3d_aware else oc, oc, 3, padding=1)))
        if oc == channels:
            self.skip_connection = nn.Identity()
        else:
            self.skip_connection = conv_nd(dims, channels, oc, 3 if use_conv else 1, padding=1 if use_conv else 0)


class QKVAttention(nn.Module):
    pass


class AttentionBlock(nn.Module):
    def __init__(self, channels, num_heads=1, use_checkpoint=False):
        super().__init__()
        self.channels, self.num_heads = channels, num_heads
        self.norm = normalization(channels)
        self.qkv = conv_nd(1, channels, channels * 3, 1)
        self.attention = QKVAttention()
        self.proj_out = zero_module(conv_nd(1, channels, channels, 1))


class _GEGLU(nn.Module):
    def __init__(self, dim_in, dim_out):
        super().__init__()
        self.proj = nn.Linear(dim_in, dim_out * 2)


class _FeedForward(nn.Module):
    def __init__(self, dim, mult=4):
        super().__init__()
        self.net = nn.Sequential(_GEGLU(dim, dim * mult), nn.Dropout(0.0), nn.Linear(dim * mult, dim))


class _CrossAttention(nn.Module):
    def __init__(self, query_dim, context_dim=None, heads=8, dim_head=64):
        super().__init__()
        inner = dim_head * heads
        self.heads, self.scale = heads, dim_head ** -0.5
        self.to_q = nn.Linear(query_dim, inner, bias=False)
        self.to_k = nn.Linear(context_dim or query_dim, inner, bias=False)
        self.to_v = nn.Linear(context_dim or query_dim, inner, bias=False)
        self.to_out = nn.Sequential(nn.Linear(inner, query_dim), nn.Dropout(0.0))


class _BasicTransformerBlock(nn.Module):
    def __init__(self, dim, n_heads, d_head, context_dim=None):
        super().__init__()
        self.attn1 = _CrossAttention(dim, heads=n_heads, dim_head=d_head)
        self.ff = _FeedForward(dim)
        self.attn2 = _CrossAttention(dim, context_dim=context_dim, heads=n_heads, dim_head=d_head)
        self.norm1, self.norm2, self.norm3 = nn.LayerNorm(dim), nn.LayerNorm(dim), nn.LayerNorm(dim)


class SpatialTransformer(nn.Module):
    """Parameter holder with the reference's layout (spatial_transformer.py:136-178); the math runs in hl_unet_forward."""

    def __init__(self, in_channels, n_heads, d_head, depth=1, dropout=0.0, context_dim=None):
        super().__init__()
        if depth != 1 or dropout != 0:
            raise NotImplementedError("SpatialTransformer: depth 1, dropout 0 (the reference's defaults)")
        self.in_channels, self.n_heads, self.d_head = in_channels, n_heads, d_head
        inner = n_heads * d_head
        assert inner == in_channels, "unet.py builds it with d_head = ch // num_heads"
        self.norm = nn.GroupNorm(32, in_channels, eps=1e-6, affine=True)
        self.proj_in = nn.Conv2d(in_channels, inner, 1)
        self.transformer_blocks = nn.ModuleList([_BasicTransformerBlock(inner, n_heads, d_head, context_dim=context_dim)])
        self.proj_out = zero_module(nn.Conv2d(inner, in_channels, 1))


def _attn_layer(ch, heads, xf_ctx):
    return SpatialTransformer(ch, heads, ch // heads, context_dim=xf_ctx) if xf_ctx else AttentionBlock(ch, num_heads=heads)


def _encoder(in_channels, mc, channel_mult, num_res_blocks, attention_resolutions, emb_dim, dropout, dims, heads, aware=False, xf_ctx=None, ssn=True):
    """Block list of one encoder tower + its per-block channel counts (unet.py:375-415 / 477-518)."""
    blocks = [TimestepEmbedSequential(conv_nd(dims, in_channels, mc, 3, padding=1))]
    chans, ch, ds = [mc], mc, 1
    for level, mult in enumerate(channel_mult):
        for _ in range(num_res_blocks):
            layers = [ResBlock(ch, emb_dim, dropout, out_channels=mult * mc, dims=dims, use_scale_shift_norm=ssn, use_3d_aware=aware)]
            ch = mult * mc
            if ds in attention_resolutions:
                layers.append(_attn_layer(ch, heads, xf_ctx))
            blocks.append(TimestepEmbedSequential(*layers))
            chans.append(ch)
        if level != len(channel_mult) - 1:
            blocks.append(TimestepEmbedSequential(Downsample(ch, True, dims=dims)))
            chans.append(ch)
            ds *= 2
    return blocks, chans, ch, ds


class UNetModel(nn.Module):
    def __init__(self, in_channels, model_channels, out_channels, num_res_blocks, attention_resolutions, dropout=0,
                 channel_mult=(1, 2, 4, 8), conv_resample=True, dims=2, num_classes=None, use_checkpoint=False,
                 num_heads=1, num_heads_upsample=-1, use_scale_shift_norm=False, cond_type="", use_3d_aware=False,
                 transformer_depth=1, context_dim=None):
        super().__init__()
        if num_heads_upsample == -1:
            num_heads_upsample = num_heads
        if dims != 2 or not conv_resample or cond_type not in ("controlnet", "", "concat", "AdaGN", "cross_attention") or \
                (use_3d_aware and cond_type in ("AdaGN", "cross_attention")):
            raise NotImplementedError(
                "the MI355X build covers dims=2, conv_resample=True, cond_type in {'controlnet', '', 'concat', "
                "'AdaGN', 'cross_attention'}, use_3d_aware with 'controlnet' / '' / 'concat' (the shipped HumanLiff configuration is controlnet, "
                "use_3d_aware=False)")
        # dropout (unet.py:196: nn.Dropout in out_layers) acts in the training path only (unet_train.py); sampling is eval-mode = identity
        self.in_channels, self.model_channels, self.out_channels = in_channels, model_channels, out_channels
        self.num_res_blocks = num_res_blocks
        self.attention_resolutions = tuple(attention_resolutions)
        self.dropout, self.channel_mult, self.conv_resample = dropout, tuple(channel_mult), conv_resample
        self.num_classes, self.use_checkpoint = num_classes, use_checkpoint
        self.num_heads, self.num_heads_upsample = num_heads, num_heads_upsample
        self.cond_type, self.use_3d_aware, self.use_scale_shift_norm = cond_type, use_3d_aware, use_scale_shift_norm

        emb_dim = model_channels * 4
        self.time_embed = nn.Sequential(linear(model_channels, emb_dim), SiLU(), linear(emb_dim, emb_dim))
        if num_classes is not None:
            self.label_emb = nn.Embedding(num_classes, emb_dim)
        xf_ctx = emb_dim if cond_type == "cross_attention" else None      # unet.py:364: context_dim = model_channels * 4
        if transformer_depth != 1:
            raise NotImplementedError("transformer_depth != 1")
        enc, chans, ch, ds = _encoder(in_channels, model_channels, self.channel_mult, num_res_blocks,
                                      self.attention_resolutions, emb_dim, dropout, dims, num_heads, aware=use_3d_aware, xf_ctx=xf_ctx, ssn=use_scale_shift_norm)
        self.input_blocks = nn.ModuleList(enc)
        self.middle_block = TimestepEmbedSequential(
            ResBlock(ch, emb_dim, dropout, dims=dims, use_scale_shift_norm=use_scale_shift_norm, use_3d_aware=use_3d_aware),
            _attn_layer(ch, num_heads, xf_ctx),
            ResBlock(ch, emb_dim, dropout, dims=dims, use_scale_shift_norm=use_scale_shift_norm, use_3d_aware=use_3d_aware))
        self.output_blocks = nn.ModuleList([])
        stack = list(chans)
        for level, mult in list(enumerate(self.channel_mult))[::-1]:
            for i in range(num_res_blocks + 1):
                layers = [ResBlock(ch + stack.pop(), emb_dim, dropout, out_channels=model_channels * mult, dims=dims,
                                   use_scale_shift_norm=use_scale_shift_norm, use_3d_aware=use_3d_aware)]
                ch = model_channels * mult
                if ds in self.attention_resolutions:
                    layers.append(_attn_layer(ch, num_heads, xf_ctx) if xf_ctx else AttentionBlock(ch, num_heads=num_heads_upsample))
                if level and i == num_res_blocks:
                    layers.append(Upsample(ch, True, dims=dims))
                    ds //= 2
                self.output_blocks.append(TimestepEmbedSequential(*layers))
        self.out = nn.Sequential(normalization(ch), SiLU(),
                                 zero_module(conv_nd(dims, model_channels, out_channels, 3, padding=1)))
        if cond_type == "controlnet":
            cenc, cchans, _, _ = _encoder(in_channels, model_channels, self.channel_mult, num_res_blocks,
                                          self.attention_resolutions, emb_dim, dropout, dims, num_heads, ssn=use_scale_shift_norm)
            self.input_blocks_cond = nn.ModuleList(cenc)
            self.input_blocks_proj_cond = nn.ModuleList(
                [zero_module(conv_nd(dims, c, c, 1, padding=0)) for c in cchans])
        elif cond_type in ("AdaGN", "cross_attention"):   # unet.py:519-525: the condition becomes one more summand of the timestep embedding / the context token
            self.conv_proj_1 = conv_nd(dims, self.out_channels, 6, 3, padding=1, stride=2)
            self.conv_proj_2 = conv_nd(dims, 6, 1, 3, padding=1, stride=2)
            self.linear = nn.Linear(64 * 64, emb_dim)
        self._hip = None       # (handle, packed buffer, key)
        self._conv_mode = _lib.HL_CONV_FP32
        self._ws = {}          # (B,H,W,device) -> workspace tensor

    # ---- reference API kept for callers ----------------------------------------------------------
    @property
    def inner_dtype(self):
        return next(self.input_blocks.parameters()).dtype

    def convert_to_fp16(self):
        raise NotImplementedError("fp16 torso is a training feature of the reference; this build computes in fp32")

    def convert_to_fp32(self):
        return None

    # ---- HIP binding -------------------------------------------------------------------------------
    def _cfg(self):
        c = _lib.UNetCfg()
        c.in_channels, c.model_channels, c.out_channels = self.in_channels, self.model_channels, self.out_channels
        c.num_res_blocks = self.num_res_blocks
        c.n_levels = len(self.channel_mult)
        for i, m in enumerate(self.channel_mult):
            c.channel_mult[i] = m
        c.n_attention_ds = len(self.attention_resolutions)
        for i, d in enumerate(self.attention_resolutions):
            c.attention_ds[i] = d
        c.num_heads, c.num_heads_upsample = self.num_heads, self.num_heads_upsample
        c.num_classes = self.num_classes or 0
        c.controlnet = 1 if self.cond_type == "controlnet" else 0
        c.adagn = 1 if self.cond_type == "AdaGN" else 0
        c.no_scale_shift = 0 if self.use_scale_shift_norm else 1
        c.cross_attn = 1 if self.cond_type == "cross_attention" else 0
        c.aware3d = 1 if self.use_3d_aware else 0
        return c

    def train(self, mode=True):           # entering training mode: optimizer steps are coming (fused ones do not bump Tensor._version)
        if mode and not self.training:
            self._hip_stale = True
        return super().train(mode)

    def _apply(self, fn, *a, **kw):       # .to() / .cuda() / .float(): parameter objects may be replaced
        self._sd_cache = None
        return super()._apply(fn, *a, **kw)

    def load_state_dict(self, *a, **kw):  # assign=True replaces parameter objects
        self._sd_cache = None
        return super().load_state_dict(*a, **kw)

    def _bind(self):
        # the (name, tensor) list of the state_dict is built once; per forward only the cheap (address, version) probe runs
        sd = getattr(self, "_sd_cache", None)
        if sd is None:
            sd = self._sd_cache = dict(self.state_dict(keep_vars=True))
        # The packed copy (1.9 GB, tens of ms to build) is kept while nothing can have changed the parameters: same tensors, same
        # versions, and no training-mode forward since it was built - `torch.optim.AdamW(fused=True)` (and any raw-pointer writer)
        # updates parameters WITHOUT bumping Tensor._version, so after a training forward the next sampling call re-lays the weights.
        key = [(v.data_ptr(), v._version) for v in sd.values()]
        if self._hip is not None and self._hip[2] == key and not getattr(self, "_hip_stale", False):
            return self._hip[0]
        self._hip_stale = False
        L = _lib.lib()
        if self._hip is not None:
            L.hl_unet_destroy(self._hip[0])
            self._hip = None
        dev = None
        for k, v in sd.items():
            if not v.is_cuda:
                raise RuntimeError("UNetModel parameters must be on the GPU (model.to('cuda')); there is no CPU path")
            if v.dtype != th.float32 or not v.is_contiguous():
                raise RuntimeError(f"parameter {k} must be contiguous fp32")
            dev = v.device
        cfg = self._cfg()
        nbytes = L.hl_unet_packed_bytes(C.byref(cfg))
        if nbytes == 0:
            _lib.check(-1, "hl_unet_packed_bytes")
        packed = th.empty(nbytes // 4 + 64, dtype=th.float32, device=dev)
        n = len(sd)
        names = (C.c_char_p * n)(*[k.encode() for k in sd])
        ptrs = (C.c_void_p * n)(*[v.data_ptr() for v in sd.values()])
        numels = (C.c_int64 * n)(*[v.numel() for v in sd.values()])
        handle = C.c_void_p()
        with th.cuda.device(dev):
            _lib.check(L.hl_unet_create(C.byref(cfg), n, names, ptrs, numels, _lib.ptr(packed), _lib.stream_ptr(),
                                        C.byref(handle)), "hl_unet_create")
        _lib.check(L.hl_unet_set_conv_mode(handle, self._conv_mode), "hl_unet_set_conv_mode")
        self._hip = (handle, packed, key)
        self._ws = {}
        return handle

    def set_conv_mode(self, mode):
        """Arithmetic of the large convolutions: "fp32" (default; fp32-class products and fp32 accumulation throughout - Winograd F(4x4,3x3) / F(2x2,3x3) on the
        fp32 matrix pipe or the fp32 direct implicit GEMM where the following does not apply; since round 5 every 3x3 / stride-1 and 1x1 layer with Cout a multiple of 192
        and enough work is a direct convolution that forms its fp32 products from two fp16 planes per operand on the 16-bit matrix pipe, error of the fp32 direct kernel's class),
        "fp32_mfma" (the same dispatch with every product on v_mfma_f32_32x32x2_f32: the default of rounds 3-4), "fp32_f23" (no F(4x4,3x3)), "fp32_direct" (direct implicit GEMM only: every product
        a*b of the reference's sum is formed exactly once) or "bf16x3" (opt-in extension, not in the reference: the
        same fp32 tensors and accumulators, each product formed on the bf16 matrix pipe from exact three-way bf16
        splits of both factors, six partial products; error per product <= 3*2^-24 - fp32 class, not bit-identical) or "fp16" (opt-in:
        fp16 operands / fp32 accumulation on the 3x3 / stride-1 layers k_conv_h16 covers - the operand precision the reference's own
        convolutions have under TF32 on its hardware, 10 explicit significand bits - every other layer as "fp32").
        See include/humanliff_hip.h HL_CONV_*."""
        modes = {"fp32": _lib.HL_CONV_FP32, "fp32_mfma": _lib.HL_CONV_FP32_MFMA, "bf16x3": _lib.HL_CONV_BF16X3, "fp32_direct": _lib.HL_CONV_FP32_DIRECT, "fp32_f23": _lib.HL_CONV_FP32_F23,
                 "fp16": _lib.HL_CONV_FP16}
        if mode not in modes:
            raise ValueError(f"unknown conv mode {mode!r} (expected one of {sorted(modes)})")
        self._conv_mode = modes[mode]
        if self._hip is not None:
            _lib.check(_lib.lib().hl_unet_set_conv_mode(self._hip[0], self._conv_mode), "hl_unet_set_conv_mode")
        return self

    def dispatch_census(self):
        """Which kernel family every convolution of the LAST inference forward took (hl_unet_dispatch_census):
        {"direct" | "wino2" | "bf16x3" | "wino4" | "fp16x2": [launches per resolution level, level = log2(H / H_out)]} ("fp16x2": the direct convolutions with fp16x2
        products, k_conv_h2s / k_conv1_h2s).  Kernel selection depends
        on the batch size, so parity tests state with this which dispatch they covered."""
        if self._hip is None:
            raise RuntimeError("dispatch_census: no forward has run yet")
        counts = (C.c_int64 * 40)()
        _lib.check(_lib.lib().hl_unet_dispatch_census_ex(self._hip[0], counts, 5), "hl_unet_dispatch_census_ex")
        return {name: [int(counts[p * 8 + l]) for l in range(8)] for p, name in enumerate(("direct", "wino2", "bf16x3", "wino4", "fp16x2"))}

    def __del__(self):
        try:
            if self._hip is not None:
                _lib.lib().hl_unet_destroy(self._hip[0])
        except Exception:
            pass

    def _any_param_requires_grad(self):
        return any(p.requires_grad for p in self.parameters())

    def forward(self, x, timesteps, x_cond=None, y=None):
        """Same contract as the reference: x (N,C,H,W), timesteps (N,), x_cond (N,C,H,W), y (N,) -> (N,C_out,H,W)."""
        if self.num_classes is not None:
            assert y is not None and y.shape == (x.shape[0],)
        if self.cond_type in ("controlnet", "AdaGN", "cross_attention"):
            assert x_cond is not None, f"cond_type='{self.cond_type}' needs x_cond (zeros for the first layer)"
        if self.cond_type == "concat":        # unet.py:572-573: the condition rides along as extra input channels (in_channels counts both)
            assert x_cond is not None, "cond_type='concat' needs x_cond"
            if self.use_3d_aware:
                # unet.py:566-573 rolls the planes of x and of x_cond out separately, (B, C/3, H, 3W) each, and only then joins the
                # channels: plane p of the network input is [x_p | cond_p].  The kernels cut the joined tensor into three equal channel
                # ranges, so the join is made per plane here.
                B_, Cx, H_, W_ = x.shape
                Cc_ = x_cond.shape[1]
                assert Cx % 3 == 0 and Cc_ % 3 == 0, (Cx, Cc_)
                x = th.cat([x.reshape(B_, 3, Cx // 3, H_, W_), x_cond.reshape(B_, 3, Cc_ // 3, H_, W_)], dim=2).reshape(B_, Cx + Cc_, H_, W_)
                x_cond = None
            else:
                x, x_cond = th.cat([x, x_cond], dim=1), None
        if not x.is_cuda:
            raise RuntimeError("UNetModel.forward needs CUDA(HIP) tensors; there is no CPU path")
        # Which path: parameter gradients are wanted in training mode only (a sampling call on a model whose parameters merely have
        # requires_grad=True - the default of a fresh module - stays on the inference kernels); a gradient with respect to x (guidance /
        # cond_fn callers) is honoured in eval mode too instead of being dropped silently.
        if th.is_grad_enabled() and (x.requires_grad or (self.training and self._any_param_requires_grad())):
            # training call (train_util.py:236 reaches this through the DDP wrapper): gradients are wanted, take the differentiable path -
            # the same network as a chain of autograd.Functions whose forward and backward are HIP kernels (unet_train.py).
            # Sampling never gets here: the loops run under no_grad and the scripts call model.eval()
            from .unet_train import forward_train
            if self.training and self._any_param_requires_grad():
                # an optimizer step follows; fused optimizers do not bump Tensor._version (see _bind).  A guidance call (eval mode, gradient
                # with respect to x only) leaves the parameters alone: the packed copies stay valid and the next sampling call does not re-pack
                self._hip_stale = True
            return forward_train(self, x, timesteps, x_cond, y)
        handle = self._bind()
        L = _lib.lib()
        B, Cc, H, W = x.shape
        planes = 3 if self.use_3d_aware else 1     # use_3d_aware: x / x_cond / the output carry the three planes as 3*in_channels channels
        assert Cc == planes * self.in_channels, (Cc, self.in_channels, self.use_3d_aware)
        xin = x.detach().to(th.float32).contiguous()
        xc = x_cond.detach().to(th.float32).contiguous() if x_cond is not None else None
        ti = tf = None
        if timesteps.is_floating_point():
            tf = timesteps.to(th.float32).contiguous()
        else:
            ti = timesteps.to(th.int64).contiguous()
        yi = y.to(th.int64).contiguous() if y is not None else None
        out = th.empty((B, planes * self.out_channels, H, W), dtype=th.float32, device=x.device)
        wkey = (B, H, W, str(x.device))
        ws = self._ws.get(wkey)
        if ws is None:
            nbytes = L.hl_unet_workspace_bytes(handle, B, H, W)
            self._ws.clear()
            ws = self._ws[wkey] = th.empty(nbytes // 4 + 64, dtype=th.float32, device=x.device)
        with th.cuda.device(x.device):
            _lib.check(L.hl_unet_forward(handle, _lib.ptr(xin), _lib.ptr(ti), _lib.ptr(tf), _lib.ptr(xc), _lib.ptr(yi),
                                         _lib.ptr(out), B, H, W, _lib.ptr(ws), _lib.stream_ptr()), "hl_unet_forward")
        return out.to(x.dtype)
