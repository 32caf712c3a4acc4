"""The attention's work-item indexing: a 1-D grid mapped to (image, head, query tile) per XCD (hl_xcd_map.h) in every attention kernel, and two query tiles per
workgroup at head size 96 (k_attention_ks<96, 4, true, true, 2>).  Neither may change a bit of the result: every shape is run with one and with two query tiles per
workgroup, placed and in launch order (hl_debug_set_attention_tiling), and compared with torch.equal, and against float64 softmax attention at the bound of
tests/test_unet_gpu.py::test_attention_matches_torch."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
dev = torch.device("cuda:0")

# (N, T, C, heads): the smallest shapes at which the indexing can go wrong
SHAPES = [
    (1, 64, 384, 4),      # one query tile: the pair has no second tile; 4 blocks < 8 XCDs
    (3, 96, 384, 4),      # odd tile count, 12 heads, 36 blocks: remainder r8 != 0
    (1, 100, 384, 4),     # a ragged last tile that is also the missing half of a pair
    (5, 160, 384, 4),     # 100 blocks: not a multiple of 8
    (1, 64, 768, 4),      # head size 192 on two key tiles: two of the four waves have no keys
    (3, 72, 768, 4),      # ... ragged
    (16, 1024, 384, 4),   # the dispatch rule itself takes two query tiles per workgroup here
]
TILINGS = [(1, 1), (1, 2), (2, 1), (2, 2)]    # (query tiles per workgroup at head size 96, XCD placement 1 off / 2 on); (0, 0) is the dispatch rule


@functools.lru_cache(maxsize=None)
def _case(N, T, C, heads):
    """qkv (N, 3C, T) as the reference lays it out, and float64 softmax attention of it (computed once per shape, on the device)."""
    g = torch.Generator().manual_seed(1000 * N + T + C)
    qkv = torch.randn((N, 3 * C, T), generator=g)
    ch = C // heads
    q, k, v = qkv.to(dev).double().reshape(N * heads, 3 * ch, T).split(ch, dim=1)
    s = 1.0 / (ch ** 0.25)
    want = torch.einsum("bts,bcs->bct", torch.softmax(torch.einsum("bct,bcs->bts", q * s, k * s), dim=-1), v).reshape(N, C, T)
    return qkv, want.cpu()


def _run(qkv, heads, h2, tiling=(0, 0)):
    from humanliff_amd import _lib
    N, C3, T = qkv.shape
    C = C3 // 3
    qd = qkv.permute(0, 2, 1).contiguous().to(dev)          # (N, T, 3C)
    out = torch.empty((N, T, C), device=dev)
    L = _lib.lib()
    _lib.check(L.hl_debug_set_attention_tiling(*tiling))
    try:
        if h2:
            _lib.check(L.hl_attention_nhwc_mode(_lib.HL_CONV_FP32, _lib.ptr(qd), N, T, C, heads, _lib.ptr(out), _lib.stream_ptr()))
        else:
            _lib.check(L.hl_attention_nhwc(_lib.ptr(qd), N, T, C, heads, _lib.ptr(out), _lib.stream_ptr()))
        torch.cuda.synchronize()
    finally:
        _lib.check(L.hl_debug_set_attention_tiling(0, 0))
    return out.cpu().permute(0, 2, 1)


@pytest.mark.parametrize("N,T,C,heads", SHAPES)
def test_attention_tilings_match_float64_and_each_other(N, T, C, heads):
    qkv, want = _case(N, T, C, heads)
    outs = {}
    for h2 in (True, False):
        for tiling in [(0, 0)] + (TILINGS if h2 else [(0, 1), (0, 2)]):
            got = _run(qkv, heads, h2, tiling)
            err = float((got.double() - want).abs().max())
            print(f"attention N{N} T{T} C{C} h2={h2} tiling={tiling}: max-abs {err:.2e}")
            assert err < 2e-5, (h2, tiling)
            outs[h2, tiling] = got
    # two runs of one tiling, and every tiling against every other: the same bits
    assert torch.equal(_run(qkv, heads, True), outs[True, (0, 0)])
    assert torch.equal(_run(qkv, heads, False), outs[False, (0, 0)])
    for tiling in [(0, 1), (0, 2)]:
        assert torch.equal(outs[False, tiling], outs[False, (0, 0)]), tiling
    for tiling in TILINGS:
        assert torch.equal(_run(qkv, heads, True, tiling), outs[True, tiling]), tiling
        assert torch.equal(outs[True, tiling], outs[True, (0, 0)]), tiling


@pytest.mark.parametrize("tiling", [(0, 0)] + TILINGS)
def test_attention_tilings_follow_the_scale_of_v(tiling):
    """V x 2^k scales the exact result by 2^k; the running V scale makes the fp16x2 kernel follow bit for bit
    (tests/test_unet_gpu.py::test_attention_fp16x2_is_invariant_to_the_scale_of_v), whichever tiling runs."""
    N, T, C, heads = 3, 96, 384, 4
    base, _ = _case(N, T, C, heads)
    ch = C // heads
    ref = _run(base, heads, True, tiling)
    for kexp in (-14, -10, -6, 5, 10):
        scaled = base.clone().reshape(N * heads, 3 * ch, T)
        scaled[:, 2 * ch:] *= 2.0 ** kexp
        got = _run(scaled.reshape(N, 3 * C, T), heads, True, tiling)
        assert torch.equal(got * 2.0 ** -kexp, ref), kexp
