"""The scratch contract of the single-op convolutions (hl_conv2d_nhwc_mode / _gn / _bwd_data): the query is the whole contract.  Exactly
the queried bytes are enough, more changes nothing (torch.equal), and 256 bytes less is an argument refusal that names the query and
launches nothing."""
import pytest
import torch

pytestmark = pytest.mark.gpu
dev = torch.device("cuda:0")


def _operands(seed, N, H, W, C, Cout, ks):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((N, H, W, C), generator=g)
    w = torch.randn((Cout, C, ks, ks), generator=g) / (C * ks * ks) ** 0.5
    b = torch.randn((Cout,), generator=g)
    cA, cB = torch.rand((N, C), generator=g) + 0.5, torch.randn((N, C), generator=g) * 0.1
    return [t.to(dev) for t in (x, w, b, cA, cB)]


def _forward(N, C, H, W, Cout, ks, gn, fused=False):
    """hl_conv2d_nhwc_mode (fused: hl_conv2d_nhwc_gn) in the default mode -> (query, bytes -> (status, outputs))."""
    from humanliff_amd import _lib
    L = _lib.lib()
    x, w, b, cA, cB = _operands(N + C + Cout, N, H, W, C, Cout, ks)
    gamma, beta = torch.ones(Cout, device=dev), torch.zeros(Cout, device=dev)
    query = "hl_conv2d_gn_scratch_bytes" if fused else "hl_conv2d_scratch_bytes"
    need = getattr(L, query)(_lib.HL_CONV_FP32, N, H, W, C, Cout, ks, 1, 0, int(gn))

    def call(nbytes):
        scratch = torch.empty(nbytes // 4, device=dev)
        outs = [torch.full((N, H, W, Cout), -7.0, device=dev)]
        head = (_lib.HL_CONV_FP32, _lib.ptr(x), N, H, W, C, _lib.ptr(w), _lib.ptr(b), Cout, ks, 1, 0, _lib.ptr(cA) if gn else None,
                _lib.ptr(cB) if gn else None, 1 if gn else 0, None, _lib.ptr(outs[0]))
        if fused:
            outs += [torch.full((N, Cout), -7.0, device=dev), torch.full((N, Cout), -7.0, device=dev)]
            rc = L.hl_conv2d_nhwc_gn(*head, _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(outs[1]), _lib.ptr(outs[2]), None, _lib.ptr(scratch), nbytes,
                                     _lib.stream_ptr())
        else:
            rc = L.hl_conv2d_nhwc_mode(*head, _lib.ptr(scratch), nbytes, _lib.stream_ptr())
        torch.cuda.synchronize()
        return rc, outs
    return query, need, call


def _backward(N, Ho, Wo, C, stride, ups):
    """hl_conv2d_nhwc_bwd_data of a 3x3 convolution C -> C from dy (N,Ho,Wo,C), in the default mode."""
    from humanliff_amd import _lib
    L = _lib.lib()
    dy, w, _, _, _ = _operands(N + Ho + stride, N, Ho, Wo, C, C, 3)
    H, W = (2 * Ho, 2 * Wo) if stride == 2 else (Ho // 2, Wo // 2) if ups else (Ho, Wo)
    need = L.hl_conv2d_bwd_data_scratch_bytes(_lib.HL_CONV_FP32, N, Ho, Wo, C, C, C, 3, stride, ups, C)

    def call(nbytes):
        scratch = torch.empty(nbytes // 4, device=dev)
        dx = torch.full((N, H, W, C), -7.0, device=dev)
        rc = L.hl_conv2d_nhwc_bwd_data(_lib.HL_CONV_FP32, _lib.ptr(dy), N, Ho, Wo, C, _lib.ptr(w), C, C, 3, stride, ups, _lib.ptr(dx), C,
                                       _lib.ptr(scratch), nbytes, _lib.stream_ptr())
        torch.cuda.synchronize()
        return rc, [dx]
    return "hl_conv2d_bwd_data_scratch_bytes", need, call


CASES = {
    "qkv_1x1_8x8": lambda: _forward(2, 384, 8, 8, 1152, 1, False),
    "3x3_8x8": lambda: _forward(4, 768, 8, 8, 768, 3, False),
    "groupnorm_input": lambda: _forward(2, 192, 32, 32, 192, 3, True),
    "fused_output_groupnorm": lambda: _forward(2, 64, 16, 16, 64, 3, False, fused=True),
    "backward_data_stride2": lambda: _backward(2, 8, 8, 64, 2, 0),
    "backward_data_upsample": lambda: _backward(2, 16, 16, 64, 1, 1),
    "raw_input_fp16x2": lambda: _forward(4, 384, 32, 32, 1152, 1, False),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_conv_scratch_query_is_the_contract(case):
    from humanliff_amd import _lib
    L = _lib.lib()
    query, need, call = CASES[case]()
    assert need % 256 == 0
    rc, exact = call(need)
    assert rc == 0, L.hl_last_error()
    assert all(bool(torch.isfinite(t).all()) and not bool((t == -7.0).all()) for t in exact)
    rc, roomy = call(2 * need)
    assert rc == 0, L.hl_last_error()
    assert all(torch.equal(a, b) for a, b in zip(exact, roomy))                  # slack changes nothing
    rc, short = call(need - 256)
    msg = L.hl_last_error().decode()
    assert rc == -1 and query in msg and str(need - 256) in msg and str(need) in msg, msg
    assert all(bool((t == -7.0).all()) for t in short)                           # refused before anything was launched
