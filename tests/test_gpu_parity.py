"""GPU parity tests: the HIP path (through the C-ABI) against the CPU oracle and against the
golden vectors produced by the real reference.  Tolerances (float32 path):
  * single conv / GEMM launches:   1e-5 relative to the output scale
  * backbone features, parameters, vertices, joints, measurements: 1e-4 absolute
    (the bar BASELINE.json states: "within 1e-4 fp32 on identical inputs")
  * mesh-mesh intersection op: bit-exact faces and barycentrics vs the C oracle
"""
import ctypes
import os
import os.path as osp

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
DATA = osp.join(ROOT, 'shapy_amd', 'data')
SUB = 7


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')


@pytest.fixture(scope='module')
def lib():
    _need_gpu()
    from shapy_amd import _lib
    return _lib.load()


def _conv_call(lib, x, w, b, res=None, relu=False, stride=1, pad=0, ups=1, tile=0, out=None,
               out_ld=None, out_coff=0, x6=False, wino=False, ksplit=1, split_bufs=None):
    """x [B,H,W,C] NHWC cuda, w [O,kh,kw,C] cuda -> out NHWC."""
    from shapy_amd import _lib
    B, Hi, Wi, C = x.shape
    O, ks = w.shape[0], w.shape[1]
    Ho = (Hi + 2 * pad - ks) // stride + 1
    Wo = (Wi + 2 * pad - ks) // stride + 1
    if out is None:
        out = torch.empty(B, Ho * ups, Wo * ups, O, device=x.device, dtype=x.dtype)
    d = _lib.ShapyConv()
    d.dtype = _lib.DTYPE_BF16 if x.dtype == torch.bfloat16 else _lib.DTYPE_F32
    wq = w
    if x6:                                             # weights as three bf16 planes [O,3,Kp]
        from shapy_amd.utils.split import split_bf16x3
        d.dtype = _lib.DTYPE_F32X6
        wq = torch.from_numpy(split_bf16x3(w.cpu().numpy().reshape(O, -1)).view(np.int16)).to(x.device)
    d.in_ = x.data_ptr(); d.wgt = wq.data_ptr(); d.bias = b.data_ptr() if b is not None else None
    d.res = res.data_ptr() if res is not None else None
    d.out = out.data_ptr()
    d.B, d.Hi, d.Wi, d.Cin, d.in_ld = B, Hi, Wi, C, C
    d.Ho, d.Wo, d.Cout = Ho, Wo, O
    d.ksize, d.stride, d.pad = ks, stride, pad
    d.out_ld = out_ld or O; d.out_coff = out_coff
    d.res_ld = (out_ld or O) if res is not None else 0; d.res_coff = out_coff if res is not None else 0
    d.relu = int(relu); d.ups = ups; d.tile = tile
    if wino == 4:                                      # F(4x4,3x3) filters (conv_wino4.hip)
        from shapy_amd.utils import winograd
        wu = torch.from_numpy(winograd.transform_filters4(w.cpu().numpy())).to(x.device)
        d.wgt_wino = wu.data_ptr()
        d.tile = tile | _lib.TILE_WINO4
        if ksplit > 1:                                 # split-K: slab + zeroed counters from the caller
            slab, ncnt = _lib.w4_split_sizes(Hi, Wi, O, ksplit)
            if split_bufs is None:
                split_bufs = (torch.full((slab * B,), float('nan'), device=x.device),
                              torch.zeros(ncnt * B, dtype=torch.int32, device=x.device))
    elif wino:                                         # Winograd-transformed filters as well
        from shapy_amd.utils import winograd
        wu = torch.from_numpy(winograd.transform_filters(w.cpu().numpy())).to(x.device)
        d.wgt_wino = wu.data_ptr()
    if ksplit > 1:
        if split_bufs is None:                         # implicit-GEMM split-K (no F(4x4) filters given)
            slab, ncnt = _lib.igemm_split_sizes(Ho, Wo, O, ksplit)
            split_bufs = (torch.full((slab * B,), float('nan'), device=x.device),
                          torch.zeros(ncnt * B, dtype=torch.int32, device=x.device))
        d.split_ws, d.split_cnt = split_bufs[0].data_ptr(), split_bufs[1].data_ptr()
        d.split_kib, d.split_cnt_n = split_bufs[0].numel() * 4 // 1024, split_bufs[1].numel()
        d.tile |= _lib.tile_w4_ksplit(ksplit)
    rc = lib.shapy_conv2d(ctypes.byref(d), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out


def _conv_ref(x, w, b, res=None, relu=False, stride=1, pad=0, ups=1):
    """float64 CPU reference on NHWC tensors."""
    xc = x.detach().cpu().double().permute(0, 3, 1, 2)
    wc = w.detach().cpu().double().permute(0, 3, 1, 2)
    y = torch.nn.functional.conv2d(xc, wc, b.detach().cpu().double() if b is not None else None,
                                   stride, pad)
    if ups > 1:
        y = torch.nn.functional.interpolate(y, scale_factor=ups, mode='nearest')
    y = y.permute(0, 2, 3, 1)
    if res is not None:
        y = y + res.detach().cpu().double()
    if relu:
        y = y.clamp_min(0)
    return y


CONV_CASES = [
    # B, H, W, Cin, Cout, ks, stride, ups, res, relu, tile
    (2, 12, 12, 48, 48, 3, 1, 1, True, True, 0),
    (2, 12, 12, 48, 48, 3, 1, 1, True, True, 1),      # 256x48
    (2, 12, 12, 48, 48, 3, 1, 1, False, True, 5),     # 64x48
    (3, 10, 14, 96, 96, 3, 1, 1, True, True, 2),      # 128x96
    (3, 10, 14, 96, 96, 3, 1, 1, True, False, 6),     # 64x96
    (2, 9, 9, 64, 256, 1, 1, 1, False, False, 3),     # 128x128 1x1
    (2, 9, 9, 256, 64, 1, 1, 1, False, True, 4),      # 256x64
    (2, 9, 9, 256, 64, 1, 1, 1, False, True, 8),      # 64x64
    (1, 7, 7, 512, 2048, 1, 1, 1, True, True, 7),     # 64x128
    (2, 16, 16, 64, 64, 3, 2, 1, False, True, 0),     # stride 2
    (2, 15, 13, 96, 192, 3, 2, 1, False, True, 0),    # stride 2, odd size
    (2, 4, 4, 192, 48, 1, 1, 4, True, True, 0),       # fuse: 1x1 + nearest x4 + add + relu
    (2, 5, 5, 96, 48, 1, 1, 2, True, False, 0),       # fuse: x2, no relu
    (2, 3, 3, 384, 48, 1, 1, 8, True, True, 5),       # fuse: x8
    (5, 1, 1, 496, 1000, 1, 1, 1, True, False, 0),    # GEMM with N tail, M tail
    (4, 1, 1, 32, 31425, 1, 1, 1, False, False, 0),   # blend-shape GEMM shape
    (2, 7, 7, 192, 192, 3, 1, 1, True, True, 11),     # 32x64 (few M tiles), M tail
    (1, 7, 7, 512, 2048, 1, 1, 1, True, True, 11),    # 32x64, 1x1
]


@pytest.mark.parametrize('case', CONV_CASES, ids=[str(c) for c in CONV_CASES])
def test_conv_kernel_vs_float64(lib, case):
    B, H, W, Cin, Cout, ks, stride, ups, use_res, relu, tile = case
    g = torch.Generator().manual_seed(hash(case) % (2 ** 31))
    x = torch.randn(B, H, W, Cin, generator=g).cuda()
    w = (torch.randn(Cout, ks, ks, Cin, generator=g) / np.sqrt(ks * ks * Cin)).cuda()
    b = torch.randn(Cout, generator=g).cuda()
    pad = ks // 2
    Ho = (H + 2 * pad - ks) // stride + 1
    Wo = (W + 2 * pad - ks) // stride + 1
    res = torch.randn(B, Ho * ups, Wo * ups, Cout, generator=g).cuda() if use_res else None
    out = _conv_call(lib, x, w, b, res, relu, stride, pad, ups, tile)
    ref = _conv_ref(x, w, b, res, relu, stride, pad, ups)
    err = (out.cpu().double() - ref).abs().max().item()
    assert err < 2e-5, err


WINO_CASES = [
    # B, H, W, Cin, Cout, res, relu
    (1, 4, 4, 16, 48, False, False),       # 4 tiles: one partial workgroup, one K chunk
    (2, 8, 8, 16, 48, False, False),
    (1, 7, 7, 32, 96, True, False),        # odd size (masked last row / column), 2 N blocks
    (3, 14, 14, 48, 48, True, True),       # the 56x56-branch layer class
    (2, 5, 6, 16, 48, False, True),
    (2, 28, 28, 96, 96, True, True),
    (1, 14, 14, 192, 192, True, True),
    (1, 7, 7, 384, 384, True, True),
    (2, 56, 56, 48, 48, True, True),
    (2, 12, 12, 64, 64, True, True),       # 64-channel N tiles (layer1's 64 -> 64)
    (1, 7, 7, 512, 512, False, True),      # the head's 512 -> 512
    (2, 9, 9, 32, 128, True, False),
    (1, 6, 6, 48, 48, False, False),       # all-K staging (Cin = 48), no residual, partial workgroup
    (2, 10, 10, 48, 96, True, True),       # all-K staging, 2 N blocks
    (1, 5, 7, 64, 128, False, True),       # all-K staging of the 64-wide variant (Cin = 64)
]


@pytest.mark.parametrize('tm', [1, 2])
@pytest.mark.parametrize('case', WINO_CASES, ids=[str(c) for c in WINO_CASES])
def test_conv_winograd_kernel_vs_float64(lib, case, tm):
    """csrc/conv_wino.hip through shapy_conv2d (ShapyConv.wgt_wino) against float64, and
    against the direct kernel on the same operands."""
    B, H, W, Cin, Cout, use_res, relu = case
    g = torch.Generator().manual_seed(hash(case) % (2 ** 31))
    x = torch.randn(B, H, W, Cin, generator=g).cuda()
    w = (torch.randn(Cout, 3, 3, Cin, generator=g) / np.sqrt(9 * Cin)).cuda()
    b = torch.randn(Cout, generator=g).cuda()
    res = torch.randn(B, H, W, Cout, generator=g).cuda() if use_res else None
    out = _conv_call(lib, x, w, b, res, relu, 1, 1, tile=0x4000 * tm, wino=True)   # 16 tm tiles / WG
    direct = _conv_call(lib, x, w, b, res, relu, 1, 1, tile=0x2000, wino=True)   # forced direct
    ref = _conv_ref(x, w, b, res, relu, 1, 1)
    e = (out.cpu().double() - ref).abs()
    ed = (direct.cpu().double() - ref).abs().max().item()
    if not e.max().item() < 2e-5:           # localise: which pixels / channels are off
        bad = (e > 2e-5)
        print('bad fraction', bad.float().mean().item(), 'direct err', ed)
        print('bad per row y:', bad.any(dim=3).any(dim=2).any(dim=0).int().tolist())
        print('bad per col x:', bad.any(dim=3).any(dim=1).any(dim=0).int().tolist())
        print('bad per channel:', bad.any(dim=2).any(dim=1).any(dim=0).int().tolist())
        print('bad per image:', bad.any(dim=3).any(dim=2).any(dim=1).int().tolist())
    assert ed < 2e-5, ed
    assert e.max().item() < 2e-5, e.max().item()
    assert not torch.equal(out, direct) or Cin * H * W < 300   # really a different algorithm


def test_conv_winograd_concat_offset(lib):
    """Winograd epilogue with out_ld > Cout / channel offset, in-place residual."""
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, 10, 10, 32, generator=g).cuda()
    w = (torch.randn(48, 3, 3, 32, generator=g) / 17).cuda()
    b = torch.randn(48, generator=g).cuda()
    big = torch.randn(2, 10, 10, 112, generator=g).cuda()
    before = big.clone()
    _conv_call(lib, x, w, b, res=big, relu=True, stride=1, pad=1, out=big, out_ld=112,
               out_coff=16, wino=True)
    ref = _conv_ref(x, w, b, before[..., 16:64], True, 1, 1)
    assert (big[..., 16:64].cpu().double() - ref).abs().max().item() < 2e-5
    assert torch.equal(big[..., :16], before[..., :16]) and torch.equal(big[..., 64:], before[..., 64:])


WINO4_CASES = [
    (1, 8, 8, 16, 48, False, False),       # 4 tiles: one partly filled workgroup, one K chunk
    (2, 12, 20, 48, 48, True, True),       # 30 tiles: two workgroups, the unrolled 3-chunk kernel
    (1, 7, 9, 32, 96, True, False),        # partial edge tiles (masked rows / columns), 2 N blocks
    (3, 14, 14, 48, 48, True, True),
    (2, 5, 6, 16, 48, False, True),
    (2, 28, 28, 96, 96, True, True),       # the 28x28-branch layer class (unrolled 6 chunks)
    (2, 56, 56, 48, 48, True, True),       # the 56x56-branch layer class
    (1, 56, 56, 256, 48, False, True),     # transition1: 16 chunks through the generic loop
    (1, 14, 14, 192, 192, True, True),
    (1, 7, 7, 384, 384, True, True),       # N-slab order (transformed filters > 2 MB)
    (5, 4, 4, 16, 48, False, False),       # one tile per image, 5 of 16 tiles live
    (1, 3, 3, 16, 48, True, False),        # smaller than one tile
    (2, 12, 20, 64, 96, True, True),       # four chunks through the generic loop, two N tiles
    (1, 9, 9, 80, 48, False, True),        # five chunks (odd count: both V buffers end up as the exchange buffer)
]


# split-K (csrc/conv_wino4.hip, template parameter S): B, H, W, Cin, Cout, res, relu, S
WINO4_SPLIT_CASES = [
    (64, 7, 7, 384, 384, True, True, 2),       # the 7x7 branch at the headline batch: 256 workgroups, KC = 12
    (64, 7, 7, 384, 384, True, True, 3),       # 8 chunks per slice
    (64, 7, 7, 384, 384, False, True, 4),      # 6 chunks per slice, four-term ordered sum
    (1, 7, 7, 384, 384, True, True, 2),        # 4 of 16 tiles live (dead lanes never touch the slab)
    (3, 7, 9, 96, 96, True, False, 2),         # partial edge tiles, generic chunk loop (3 chunks per slice)
    (64, 14, 14, 192, 192, True, True, 2),     # the 14x14 branch: KC = 6
    (8, 14, 14, 192, 192, True, True, 4),      # ... small-batch policy: KC = 3, four slices
    (8, 28, 28, 96, 96, True, True, 2),        # the 28x28 branch, small-batch policy: KC = 3, two slices
    (5, 7, 7, 256, 96, False, True, 2),        # 8 chunks per slice through the generic loop
]


@pytest.mark.parametrize('case', WINO4_SPLIT_CASES, ids=[str(c) for c in WINO4_SPLIT_CASES])
def test_conv_winograd4_split_k_vs_float64(lib, case):
    """F(4x4) with the K loop cut into S slices on S workgroups per output tile: against float64 and
    against the unsplit kernel (same products, the S partial sums added in slice order: float32
    rounding apart), REPEATED on the same slab / counters -- the kernel leaves its arrival counters
    zero, the result is bit-identical from launch to launch whichever slice arrives last -- and with
    a busy stream in front so that slices of a tile start at different times."""
    B, H, W, Cin, Cout, use_res, relu, S = case
    g = torch.Generator().manual_seed(hash(case) % (2 ** 31))
    x = torch.randn(B, H, W, Cin, generator=g).cuda()
    w = (torch.randn(Cout, 3, 3, Cin, generator=g) / np.sqrt(9 * Cin)).cuda()
    b = torch.randn(Cout, generator=g).cuda()
    res = torch.randn(B, H, W, Cout, generator=g).cuda() if use_res else None
    from shapy_amd import _lib
    slab, ncnt = _lib.w4_split_sizes(H, W, Cout, S)
    bufs = (torch.full((slab * B,), float('nan'), device='cuda'),
            torch.zeros(ncnt * B, dtype=torch.int32, device='cuda'))
    base = _conv_call(lib, x, w, b, res, relu, 1, 1, wino=4)
    ref = _conv_ref(x, w, b, res, relu, 1, 1)
    tol = 2e-6 * np.sqrt(9 * Cin)
    assert (base.cpu().double() - ref).abs().max().item() < tol
    outs = []
    for rep in range(6):
        if rep % 2:                     # uneven load: another kernel still running when the slices start
            junk = torch.randn(4096, 4096, device='cuda')
            junk = junk @ junk
        outs.append(_conv_call(lib, x, w, b, res, relu, 1, 1, wino=4, ksplit=S, split_bufs=bufs).clone())
        assert int(bufs[1].abs().sum().item()) == 0, 'arrival counters not back to zero'
    e = (outs[0].cpu().double() - ref).abs()
    d = (outs[0] - base).abs().max().item()
    print(f'split-K S={S}: max err vs float64 {e.max().item():.3e} (tol {tol:.1e}), vs the unsplit kernel {d:.3e}, '
          f'NaNs {int(torch.isnan(outs[0]).sum())}, launches equal {[bool(torch.equal(o, outs[0])) for o in outs[1:]]}')
    assert e.max().item() < tol, (e.max().item(), (e > tol).float().mean().item())
    assert d < tol                        # another association of the same float32 sums
    assert all(torch.equal(o, outs[0]) for o in outs[1:]), 'split-K result changes from launch to launch'


# implicit-GEMM split-K (csrc/conv_igemm.hip, SPLIT): B, H, W, Cin, Cout, ks, stride, res, relu, S, bf16
IGEMM_SPLIT_CASES = [
    (32, 7, 7, 384, 384, 3, 1, True, True, 4, True),        # the 7x7 branch in bf16 storage (configs[2] shard)
    (32, 14, 14, 192, 192, 3, 1, True, True, 2, True),      # the 14x14 branch, bf16
    (8, 7, 7, 2048, 512, 1, 1, False, True, 2, False),      # head 1x1, float32, small batch
    (3, 14, 14, 192, 384, 3, 2, True, False, 3, False),     # stride-2 fuse conv, three slices of 54 chunks
    (1, 7, 7, 512, 2048, 1, 1, True, True, 4, False),       # M tail (49 rows), N = 2048
    (5, 9, 9, 64, 64, 3, 1, False, True, 2, True),          # bf16, short K (18 chunks of 32), 64-wide tile
]


@pytest.mark.parametrize('case', IGEMM_SPLIT_CASES, ids=[str(c) for c in IGEMM_SPLIT_CASES])
def test_conv_igemm_split_k_vs_unsplit_and_float64(lib, case):
    """Split-K on the implicit-GEMM kernel: against float64 and against the unsplit launch (same products, S
    partial sums added in slice order), repeated on the same slab / counters (left zero by the kernel;
    bit-identical from launch to launch), float32 and bf16 storage."""
    B, H, W, Cin, Cout, ks, st, use_res, relu, S, bf16 = case
    dt = torch.bfloat16 if bf16 else torch.float32
    g = torch.Generator().manual_seed(hash(case) % (2 ** 31))
    x = torch.randn(B, H, W, Cin, generator=g).cuda().to(dt)
    w = (torch.randn(Cout, ks, ks, Cin, generator=g) / np.sqrt(ks * ks * Cin)).cuda().to(dt)
    b = torch.randn(Cout, generator=g).cuda()
    pad = ks // 2
    Ho, Wo = (H + 2 * pad - ks) // st + 1, (W + 2 * pad - ks) // st + 1
    res = torch.randn(B, Ho, Wo, Cout, generator=g).cuda().to(dt) if use_res else None
    from shapy_amd import _lib
    slab, ncnt = _lib.igemm_split_sizes(Ho, Wo, Cout, S)
    bufs = (torch.full((slab * B,), float('nan'), device='cuda'),
            torch.zeros(ncnt * B, dtype=torch.int32, device='cuda'))
    base = _conv_call(lib, x, w, b, res, relu, st, pad, tile=0x2000)
    ref = _conv_ref(x.float(), w.float(), b, res.float() if use_res else None, relu, st, pad)
    tol = (3e-2 if bf16 else 2e-5)
    assert (base.float().cpu().double() - ref).abs().max().item() < tol
    outs = []
    for rep in range(5):
        if rep % 2:
            junk = torch.randn(4096, 4096, device='cuda')
            junk = junk @ junk
        outs.append(_conv_call(lib, x, w, b, res, relu, st, pad, tile=0x2000, ksplit=S, split_bufs=bufs).clone())
        assert int(bufs[1].abs().sum().item()) == 0, 'arrival counters not back to zero'
    e = (outs[0].float().cpu().double() - ref).abs().max().item()
    d = (outs[0].float() - base.float()).abs().max().item()
    print(f'igemm split-K S={S} bf16={bf16}: err vs float64 {e:.3e}, vs unsplit {d:.3e}')
    assert e < tol and d < tol
    assert all(torch.equal(o, outs[0]) for o in outs[1:]), 'split-K result changes from launch to launch'


def test_conv_winograd4_split_k_refusals(lib):
    """No slab / counters, a slice count that does not divide the chunks, S on a non-F(4x4) layer."""
    from shapy_amd import _lib
    x = torch.randn(1, 7, 7, 96).cuda()
    w = torch.randn(96, 3, 3, 96).cuda()
    out = torch.full((1, 7, 7, 96), 7.0).cuda()
    from shapy_amd.utils import winograd
    wu = torch.from_numpy(winograd.transform_filters4(w.cpu().numpy())).cuda()
    slab, ncnt = _lib.w4_split_sizes(7, 7, 96, 4)
    ws, cnt = torch.zeros(slab).cuda(), torch.zeros(ncnt, dtype=torch.int32).cuda()

    def call(S, with_bufs):
        d = _lib.ShapyConv()
        d.dtype = _lib.DTYPE_F32
        d.in_, d.wgt, d.out, d.wgt_wino = x.data_ptr(), w.data_ptr(), out.data_ptr(), wu.data_ptr()
        d.B, d.Hi, d.Wi, d.Cin, d.in_ld, d.Ho, d.Wo, d.Cout = 1, 7, 7, 96, 96, 7, 7, 96
        d.ksize, d.stride, d.pad, d.out_ld, d.ups = 3, 1, 1, 96, 1
        d.tile = _lib.TILE_WINO4 | _lib.tile_w4_ksplit(S)
        if with_bufs:
            d.split_ws, d.split_cnt = ws.data_ptr(), cnt.data_ptr()
            d.split_kib, d.split_cnt_n = ws.numel() * 4 // 1024, cnt.numel()
            if with_bufs == 'small':
                d.split_kib = 1                          # a slab that is too small: refused, not overrun
        return lib.shapy_conv2d(ctypes.byref(d), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert call(2, False) == -1          # SHAPY_EINVAL: no slab
    assert call(2, 'small') == -1        # ... or one below the launch's need
    assert call(4, True) == -1           # 6 chunks do not split four ways
    torch.cuda.synchronize()
    assert torch.equal(out, torch.full_like(out, 7.0))      # nothing was launched
    assert call(2, True) == 0
    torch.cuda.synchronize()
    assert not torch.equal(out, torch.full_like(out, 7.0)) and int(cnt.abs().sum()) == 0


@pytest.mark.parametrize('case', WINO4_CASES, ids=[str(c) for c in WINO4_CASES])
def test_conv_winograd4_kernel_vs_float64(lib, case):
    """csrc/conv_wino4.hip (F(4x4,3x3), four multiplying waves that stage a quarter of every chunk each) through
    shapy_conv2d (ShapyConv.wgt_wino + SHAPY_TILE_WINO4) against float64, next to the direct
    kernel on the same operands."""
    B, H, W, Cin, Cout, use_res, relu = case
    g = torch.Generator().manual_seed(hash(case) % (2 ** 31))
    x = torch.randn(B, H, W, Cin, generator=g).cuda()
    w = (torch.randn(Cout, 3, 3, Cin, generator=g) / np.sqrt(9 * Cin)).cuda()
    b = torch.randn(Cout, generator=g).cuda()
    res = torch.randn(B, H, W, Cout, generator=g).cuda() if use_res else None
    out = _conv_call(lib, x, w, b, res, relu, 1, 1, wino=4)
    direct = _conv_call(lib, x, w, b, res, relu, 1, 1, tile=0x2000)
    ref = _conv_ref(x, w, b, res, relu, 1, 1)
    e = (out.cpu().double() - ref).abs()
    ed = (direct.cpu().double() - ref).abs().max().item()
    if not e.max().item() < 2e-6 * np.sqrt(9 * Cin):   # localise: which pixels / channels are off
        bad = (e > 2e-6 * np.sqrt(9 * Cin))
        print('bad fraction', bad.float().mean().item(), 'max', e.max().item(), 'direct err', ed)
        print('bad per row y:', bad.any(dim=3).any(dim=2).any(dim=0).int().tolist())
        print('bad per col x:', bad.any(dim=3).any(dim=1).any(dim=0).int().tolist())
        print('bad per channel:', bad.any(dim=2).any(dim=1).any(dim=0).int().tolist())
        print('bad per image:', bad.any(dim=3).any(dim=2).any(dim=1).int().tolist())
    assert ed < 2e-5, ed
    # F(4x4) transforms multiply by up to 8 (data) and 1/24 .. 1/4 (filters): on these unit-variance
    # random operands its float32 rounding is ~6x the direct sum's and grows with sqrt(K) -- first
    # GPU run: 5.1e-5 at K = 2,304, 4.7e-5 at K = 3,456, <= 2.5e-5 at K <= 864, direct 5..9e-6.
    # (On the network's real activations the F(4x4) features are as close to the CPU reference
    # as the direct ones: 4.3e-6 at bs 64, test_full_forward_bs64_vs_oracle.)  An indexing bug
    # would show up as O(1) errors.
    tol = 2e-6 * np.sqrt(9 * Cin)
    if not e.max().item() < tol:
        print('tolerance', tol)
    assert e.max().item() < tol, (e.max().item(), tol)
    assert not torch.equal(out, direct) or Cin * H * W < 300   # really a different algorithm


def test_conv_winograd4_concat_offset_and_refusals(lib):
    """F(4x4) epilogue with out_ld > Cout / channel offset and an in-place residual; layers the
    kernel does not take are refused (there is no fallback for the F(4x4) filter layout)."""
    from shapy_amd import _lib
    g = torch.Generator().manual_seed(12)
    x = torch.randn(2, 10, 10, 32, generator=g).cuda()
    w = (torch.randn(48, 3, 3, 32, generator=g) / 17).cuda()
    b = torch.randn(48, generator=g).cuda()
    big = torch.randn(2, 10, 10, 112, generator=g).cuda()
    before = big.clone()
    _conv_call(lib, x, w, b, res=big, relu=True, stride=1, pad=1, out=big, out_ld=112,
               out_coff=16, wino=4)
    ref = _conv_ref(x, w, b, before[..., 16:64], True, 1, 1)
    assert (big[..., 16:64].cpu().double() - ref).abs().max().item() < 3e-5
    assert torch.equal(big[..., :16], before[..., :16]) and torch.equal(big[..., 64:], before[..., 64:])
    # Cout = 80 / 64 have no 48-channel N tiling (64 -> 64 is an F(2x2) layer); stride 2 is not a Winograd layer
    for cout, stride in ((80, 1), (64, 1), (48, 2)):
        w2 = torch.randn(cout, 3, 3, 32, generator=g).cuda()
        d = _lib.ShapyConv()
        out = torch.empty(2, 10, 10, cout, device='cuda')
        d.in_ = x.data_ptr(); d.wgt = w2.data_ptr(); d.out = out.data_ptr()
        d.wgt_wino = w2.data_ptr()
        d.B, d.Hi, d.Wi, d.Cin, d.in_ld = 2, 10, 10, 32, 32
        d.Ho = d.Wo = (10 + 2 - 3) // stride + 1
        d.Cout, d.ksize, d.stride, d.pad = cout, 3, stride, 1
        d.out_ld = cout; d.ups = 1; d.tile = _lib.TILE_WINO4; d.dtype = _lib.DTYPE_F32
        rc = lib.shapy_conv2d(ctypes.byref(d), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc != 0, (cout, stride)


def test_conv_winograd4_falls_back_to_direct_beyond_1gib(lib):
    """The F(4x4) kernel addresses with 32-bit byte offsets and uses 0x40000000 as its "out of
    range" mark: a tensor beyond 1 GiB (here: a channel slice of a 1.08 GB concat buffer) makes
    shapy_conv2d run the direct kernel on the untransformed weights instead -- same result."""
    g = torch.Generator().manual_seed(13)
    B, H, W, C, O, LD = 21, 56, 56, 48, 48, 4096
    assert 4 * B * H * W * LD > 0x40000000
    x = torch.randn(B, H, W, C, generator=g).cuda()
    w = (torch.randn(O, 3, 3, C, generator=g) / np.sqrt(9 * C)).cuda()
    b = torch.randn(O, generator=g).cuda()
    big = torch.zeros(B, H, W, LD, device='cuda')
    _conv_call(lib, x, w, b, relu=True, stride=1, pad=1, out=big, out_ld=LD, out_coff=64, wino=4)
    direct = _conv_call(lib, x, w, b, relu=True, stride=1, pad=1, tile=0x2000)
    assert torch.equal(big[..., 64:64 + O], direct)          # the very same kernel ran
    assert not big[..., :64].any() and not big[..., 64 + O:].any()
    ref = _conv_ref(x[:2], w, b, None, True, 1, 1)
    assert (direct[:2].cpu().double() - ref).abs().max().item() < 2e-5


@pytest.mark.parametrize('kind', ['direct', 'direct_scalar', 'ups', 'winograd', 'winograd4', 'f32x6', 'bf16'])
@pytest.mark.parametrize('relu', [True, False])
def test_conv_kernels_keep_nan_through_relu(lib, kind, relu):
    """torch.relu(NaN) is NaN.  A max with zero would turn a NaN activation into 0 and hide a numerical blow-up
    from the Winograd guard and from every check downstream: every epilogue takes ReLU as compare +
    select.  One NaN in the input: each output whose receptive field holds it is NaN in every channel; the
    direct kernels leave everything else finite."""
    Cin, Cout = (48, 48) if kind == 'winograd4' else (32, 70 if kind == 'direct_scalar' else 64)
    ks = 1 if kind == 'ups' else 3
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, 12, 12, Cin, generator=g)
    x[1, 5, 6, 3] = float('nan')
    w = torch.randn(Cout, ks, ks, Cin, generator=g) / np.sqrt(ks * ks * Cin)
    b = torch.randn(Cout, generator=g)
    x, w, b = x.cuda(), w.cuda(), b.cuda()
    ups = 2 if kind == 'ups' else 1
    res = torch.randn(2, 12 * ups, 12 * ups, Cout, generator=g).cuda()
    if kind == 'bf16':
        x, w, res = x.bfloat16(), w.bfloat16(), res.bfloat16()
    out = _conv_call(lib, x, w, b, res, relu, 1, ks // 2, ups=ups, wino={'winograd': True, 'winograd4': 4}.get(kind, False),
                     x6=kind == 'f32x6').float()
    nan = torch.isnan(out)
    r = ks // 2
    field = torch.zeros_like(nan[..., 0])
    field[1, (5 - r) * ups:(5 + r + 1) * ups, (6 - r) * ups:(6 + r + 1) * ups] = True
    assert nan[field].all(), f'{int((~nan[field]).sum())} outputs lost the NaN'
    assert not nan[0].any()                                  # the other image is untouched
    if not kind.startswith('winograd'):                      # (a Winograd tile spreads it over its 2x2 / 4x4 outputs)
        assert not nan[~field].any()
    if relu:
        assert (out[~nan] >= 0).all()


X6_CASES = [c for c in CONV_CASES if c[10] in (0, 5, 8, 2, 6, 3, 7)] + [
    (2, 12, 12, 48, 48, 3, 1, 1, True, True, 8),      # Cin = 48: K chunks straddle taps
    (2, 9, 11, 20, 70, 3, 1, 1, False, False, 0),     # Cin % 32 != 0, Cin < 32, N tail
    (1, 8, 8, 4, 16, 1, 1, 1, False, False, 0),       # a single 4-wide K chunk
    (2, 12, 12, 48, 96, 3, 2, 1, False, True, 9),     # 128x48, stride 2
    (2, 12, 12, 64, 64, 3, 1, 1, True, True, 10),     # 128x64
    (4, 7, 7, 512, 1024, 1, 1, 1, True, True, 3),     # 128x128: the head's wide 1x1 GEMMs (partial M tile)
    (43, 7, 7, 512, 1024, 1, 1, 1, False, True, 0),   # ... chosen automatically from M = 2,048 on
]


@pytest.mark.parametrize('case', X6_CASES, ids=[str(c) for c in X6_CASES])
def test_conv_kernel_f32x6_vs_float64(lib, case):
    """float32 storage, products from the exact 3-way bf16 split (6 bf16 MFMAs, f32
    accumulation): same tolerance as the native f32 kernel, and the two must agree to a few
    float32 ulps of the accumulated magnitude."""
    B, H, W, Cin, Cout, ks, stride, ups, use_res, relu, tile = case
    g = torch.Generator().manual_seed(hash(case) % (2 ** 31))
    x = torch.randn(B, H, W, Cin, generator=g).cuda()
    w = (torch.randn(Cout, ks, ks, Cin, generator=g) / np.sqrt(ks * ks * Cin)).cuda()
    b = torch.randn(Cout, generator=g).cuda()
    pad = ks // 2
    Ho = (H + 2 * pad - ks) // stride + 1
    Wo = (W + 2 * pad - ks) // stride + 1
    res = torch.randn(B, Ho * ups, Wo * ups, Cout, generator=g).cuda() if use_res else None
    out = _conv_call(lib, x, w, b, res, relu, stride, pad, ups, tile, x6=True)
    ref = _conv_ref(x, w, b, res, relu, stride, pad, ups)
    err = (out.cpu().double() - ref).abs().max().item()
    assert err < 2e-5, err
    if Cin % 16 == 0:                                  # the native f32 kernel needs Cin % 16 == 0
        nat = _conv_call(lib, x, w, b, res, relu, stride, pad, ups, 0)
        assert (out - nat).abs().max().item() < 1e-5


def test_conv_f32x6_special_values(lib):
    """The split is exact for every float32 whose third part stays a normal number
    (|a| > 2^-102): huge and tiny operands, exact zeros and negative zero go through
    unchanged in value."""
    x = torch.zeros(1, 4, 4, 32)
    vals = torch.tensor([3.0e38, -1.5e-30, 1e-30, 65504.0, -0.0, 1.0 + 2.0 ** -23, 123456.789,
                         -7.0e-20])
    x.view(-1)[:8] = vals
    w = torch.zeros(16, 1, 1, 32)
    for o in range(8):
        w[o, 0, 0, o] = 1.0                           # output o copies input channel o
    w[8, 0, 0, 5] = 1.0 - 2.0 ** -24
    w[8, 0, 0, 6] = 2.0 ** -60
    out = _conv_call(lib, x.cuda(), w.cuda(), None, x6=True)
    assert torch.equal(out[0, 0, 0, :8].cpu(), vals)
    want = (vals[5].double() * w[8, 0, 0, 5].double() + vals[6].double() * w[8, 0, 0, 6].double())
    assert abs(out[0, 0, 0, 8].item() - want.item()) < 2.0 ** -23


BF16_CASES = [
    # B, H, W, Cin, Cout, ks, stride, ups, res, relu, tile
    (2, 12, 12, 64, 64, 3, 1, 1, True, True, 0),
    (3, 10, 14, 96, 96, 3, 1, 1, True, False, 0),
    (2, 9, 9, 64, 256, 1, 1, 1, False, False, 0),
    (1, 7, 7, 512, 2048, 1, 1, 1, True, True, 0),
    (2, 15, 13, 96, 192, 3, 2, 1, False, True, 0),
    (2, 4, 4, 192, 64, 1, 1, 4, True, True, 0),
    (2, 3, 3, 384, 96, 1, 1, 8, True, True, 0),
    (2, 6, 6, 32, 48, 3, 1, 1, False, True, 5),
    (2, 12, 12, 48, 48, 3, 1, 1, True, True, 0),      # flat-K kernel: Cin % 32 != 0 (unpadded 48-ch branch)
    (2, 9, 9, 48, 96, 3, 2, 1, False, True, 0),       # flat-K, stride 2
    (1, 6, 6, 48, 32, 1, 1, 1, False, False, 0),      # flat-K, 1x1, N tail
    (2, 7, 7, 40, 48, 3, 1, 1, True, False, 0),       # flat-K, Cin = 40
]


@pytest.mark.parametrize('case', BF16_CASES, ids=[str(c) for c in BF16_CASES])
def test_conv_kernel_bf16_vs_float64(lib, case):
    """bf16 storage, f32 accumulation: against float64 on the SAME bf16-rounded operands the
    only error left is the final rounding of the output to bf16 (2^-9 relative)."""
    B, H, W, Cin, Cout, ks, stride, ups, use_res, relu, tile = case
    g = torch.Generator().manual_seed(hash(case) % (2 ** 31))
    x = torch.randn(B, H, W, Cin, generator=g).bfloat16().cuda()
    w = (torch.randn(Cout, ks, ks, Cin, generator=g) / np.sqrt(ks * ks * Cin)).bfloat16().cuda()
    b = torch.randn(Cout, generator=g).cuda()
    pad = ks // 2
    Ho = (H + 2 * pad - ks) // stride + 1
    Wo = (W + 2 * pad - ks) // stride + 1
    res = torch.randn(B, Ho * ups, Wo * ups, Cout, generator=g).bfloat16().cuda() if use_res else None
    out = _conv_call(lib, x, w, b, res, relu, stride, pad, ups, tile)
    assert out.dtype == torch.bfloat16
    ref = _conv_ref(x.float(), w.float(), b, res.float() if use_res else None, relu, stride, pad, ups)
    err = (out.float().cpu().double() - ref).abs()
    tol = ref.abs() * 2.0 ** -8 + 1e-5
    assert (err <= tol).all(), float((err - tol).max())


def test_conv_concat_offset_and_inplace_residual(lib):
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 7, 7, 192, generator=g).cuda()
    w = (torch.randn(384, 3, 3, 192, generator=g) / 40).cuda()
    b = torch.randn(384, generator=g).cuda()
    cat = torch.full((2, 7, 7, 1536), 7.0).cuda()
    _conv_call(lib, x, w, b, None, True, 1, 1, 1, 0, out=cat, out_ld=1536, out_coff=768)
    ref = _conv_ref(x, w, b, None, True, 1, 1)
    assert (cat[..., 768:1152].cpu().double() - ref).abs().max() < 2e-5
    assert (cat[..., :768] == 7).all() and (cat[..., 1152:] == 7).all()
    # in-place accumulate (res == out), as used by the fuse layers
    acc0 = torch.randn(2, 7, 7, 384, generator=g).cuda()
    acc = acc0.clone()
    _conv_call(lib, x, w, b, acc, False, 1, 1, 1, 0, out=acc)
    assert (acc.cpu().double() - (ref_no_relu(x, w, b) + acc0.cpu().double())).abs().max() < 2e-5


def ref_no_relu(x, w, b):
    return _conv_ref(x, w, b, None, False, 1, 1)


# ------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def network(tmp_path_factory):
    _need_gpu()
    from shapy_amd.config import merge_config
    from shapy_amd.models import build_model
    from shapy_amd.utils import synthetic as syn
    folder = str(tmp_path_factory.mktemp('synth_models'))
    syn.write_synthetic_smplx(folder, 0)
    cfg = merge_config([osp.join(ROOT, 'configs/b2a_expose_hrnet_demo.yaml')], [
        f'body_model.model_folder={folder}',
        'network.smplx.backbone.hrnet.pretrained_path=',
        f'network.smplx.meas_definition_path={DATA}/measurement_defitions.yaml',
        f'network.smplx.meas_vertices_path={DATA}/smplx_measurements.yaml'])
    net = build_model(cfg)['network']
    syn.fill_module_synthetic(net, 0)
    net = net.to('cuda').eval()
    from shapy_amd.models.backbone import hrnet as hrnet_mod
    # the product default (smoke / bench use it; SHAPY_CONV_ALGO overrides it for A/B runs)
    assert net.backbone.conv_algo == os.environ.get('SHAPY_CONV_ALGO', hrnet_mod.DEFAULT_CONV_ALGO)
    net.backbone.conv_algo = 'direct'                  # baseline of this module: the exact-f32
    return net                                         # direct path; Winograd tests opt in


@pytest.mark.parametrize('tag,b,s', [('b2_64', 2, 64), ('b3_96', 3, 96), ('b1_224', 1, 224)])
@pytest.mark.parametrize('algo', ['winograd', 'auto'])
def test_hrnet_winograd_features_vs_reference_golden(network, golden_dir, tag, b, s, algo):
    """The float32 path with Winograd F(2x2,3x3) on the 3x3 / stride-1 layers against the
    reference's CPU features at the north-star tolerance 1e-4."""
    from shapy_amd.utils import synthetic as syn
    g = np.load(osp.join(golden_dir, 'hrnet_golden.npz'))
    x = torch.from_numpy(syn.synthetic_images(b, s, 0)).cuda()
    network.backbone.multi_stream = True
    network.backbone.conv_algo = algo
    try:
        with torch.no_grad():
            feat = network.backbone(x)['concat']
        torch.cuda.synchronize()
        eng = [e for k, e in network.backbone._engine.items() if k[4] == algo][-1]
        n_wino = sum(1 for o in eng['plan'].ops if o.get('wino_off', -1) >= 0)
    finally:
        network.backbone.conv_algo = 'direct'
    err = np.abs(feat.cpu().numpy() - g[tag]).max()
    print(tag, algo, 'winograd layers', n_wino, 'max abs err', err)
    assert n_wino > (100 if algo == 'winograd' else 0)
    assert err < 1e-4, err


@pytest.mark.parametrize('tag,b,s', [('b2_64', 2, 64), ('b3_96', 3, 96), ('b1_224', 1, 224)])
def test_hrnet_winograd4_features_vs_reference_golden(network, golden_dir, tag, b, s):
    """conv_algo = 'winograd4': F(4x4,3x3) (csrc/conv_wino4.hip) on the large maps, F(2x2,3x3) on
    the rest, against the reference's CPU features at 1e-4.  The small inputs lower the map-size
    threshold so that they, too, run F(4x4) layers (incl. partly filled tiles: 24 / 4, 12 / 4)."""
    from shapy_amd import _lib
    from shapy_amd.utils import synthetic as syn
    g = np.load(osp.join(golden_dir, 'hrnet_golden.npz'))
    x = torch.from_numpy(syn.synthetic_images(b, s, 0)).cuda()
    bb = network.backbone
    bb.multi_stream = True
    bb.conv_algo = 'winograd4'
    keep = bb.wino4_min_hw
    if s < 224:
        bb.wino4_min_hw = 6
    try:
        with torch.no_grad():
            feat = bb(x)['concat']
        torch.cuda.synchronize()
        eng = [e for k, e in bb._engine.items() if k[4] == 'winograd4' and k[0] == s][-1]
        n4 = sum(1 for o in eng['plan'].ops if o['tile'] & _lib.TILE_WINO4)
        n2 = sum(1 for o in eng['plan'].ops if o.get('wino_off', -1) >= 0) - n4
    finally:
        bb.conv_algo = 'direct'
        bb.wino4_min_hw = keep
    err = np.abs(feat.cpu().numpy() - g[tag]).max()
    print(tag, 'F(4x4) layers', n4, 'F(2x2) layers', n2, 'max abs err', err)
    assert n4 >= 100 and n2 > 0
    assert err < 1e-4, err


@pytest.mark.parametrize('tag,b,s', [('b2_64', 2, 64), ('b3_96', 3, 96), ('b1_224', 1, 224)])
@pytest.mark.parametrize('multi_stream', [False, True])
@pytest.mark.parametrize('cdt', ['f32', 'f32x6'])
def test_hrnet_features_vs_reference_golden(network, golden_dir, tag, b, s, multi_stream, cdt):
    """Both float32 arithmetic paths (native f32 MFMA, bf16x6 split) against the reference's
    CPU features at the north-star tolerance 1e-4."""
    from shapy_amd.utils import synthetic as syn
    g = np.load(osp.join(golden_dir, 'hrnet_golden.npz'))
    x = torch.from_numpy(syn.synthetic_images(b, s, 0)).cuda()
    network.backbone.multi_stream = multi_stream
    network.backbone.compute_dtype = cdt
    try:
        with torch.no_grad():
            feat = network.backbone(x)['concat']
        torch.cuda.synchronize()
    finally:
        network.backbone.compute_dtype = 'f32'
    err = np.abs(feat.cpu().numpy() - g[tag]).max()
    print(tag, cdt, 'multi_stream', multi_stream, 'max abs err', err, 'scale', np.abs(g[tag]).max())
    assert err < 1e-4, err


@pytest.mark.parametrize('multi_stream', [False, True])
def test_hrnet_graph_replay_equals_eager(network, multi_stream):
    """The hipGraph replay (default for small batches) runs the same kernels on the same
    buffers as the eager op list: bit-identical features, also on a second replay with new
    images and after an eager call in between."""
    from shapy_amd.utils import synthetic as syn
    bb = network.backbone
    bb.multi_stream = multi_stream
    xs = [torch.from_numpy(syn.synthetic_images(3, 96, seed)).cuda() for seed in (5, 6)]
    try:
        bb.use_graph = False
        with torch.no_grad():
            eager = [bb(x)['concat'].clone() for x in xs]
        bb.use_graph = True
        with torch.no_grad():
            g0 = bb(xs[0])['concat']
            g1 = bb(xs[1])['concat']
            bb.use_graph = False
            e1 = bb(xs[1])['concat']
            bb.use_graph = True
            g0b = bb(xs[0])['concat']
        torch.cuda.synchronize()
    finally:
        bb.use_graph = 'auto'
    assert torch.equal(g0, eager[0]) and torch.equal(g1, eager[1])
    assert torch.equal(e1, eager[1]) and torch.equal(g0b, eager[0])
    assert g0.data_ptr() != g0b.data_ptr()               # outputs are copies, not the baked buffer


@pytest.mark.parametrize('B,size,multi_stream,graph', [(3, 96, True, False), (2, 224, False, False),
                                                       (64, 224, True, False), (2, 64, True, True)])
def test_hrnet_grouped_branch_launches_equal_per_layer_launches(network, B, size, multi_stream, graph):
    """group_branches (the default): the convs at one depth of a module's parallel branches run as
    ONE persistent F(4x4) launch (csrc/conv_wino4g.hip, through shapy_hrnet_run's `group` ops)
    instead of one conv_wino4 launch per branch and stream -- same tasks, same products; deterministic
    from call to call, at the headline batch too, eager and as a captured hipGraph.  Against the per-layer
    kernel the features agree to float32 rounding: since round 6 the per-layer kernel adds Winograd rows 4 / 5
    of a tile in another association (its fourth wave's partial x-transform, csrc/conv_wino4.hip), as a
    split layer adds its slices' partial sums in another one -- both compared to rounding below.  (Per-layer
    launches WITHOUT split-K are the reference: the persistent kernel has no split form.)"""
    from shapy_amd.utils import synthetic as syn
    bb = network.backbone
    keep = bb.group_branches, bb.multi_stream, bb.use_graph, bb.conv_algo, bb.wino4_min_hw
    keep_split = bb.wino4_ksplit
    x = torch.from_numpy(syn.synthetic_images(B, size, 11)).cuda()
    try:
        bb.conv_algo, bb.wino4_min_hw = 'winograd4', 7
        bb.multi_stream, bb.use_graph = multi_stream, graph
        bb.group_branches = False
        with torch.no_grad():
            split = bb(x)['concat'].clone()              # the default plan: 384 @7x7 with S = 2
        bb.wino4_ksplit = {}
        with torch.no_grad():
            ref = bb(x)['concat'].clone()
        bb.group_branches = True
        with torch.no_grad():
            got = bb(x)['concat'].clone()
            again = bb(x)['concat'].clone()
        torch.cuda.synchronize()
        plan = [e for k, e in bb._engine.items() if k[7] is True][-1]['plan']
        # 224 px: every module's branch levels (8 x 2 + 32 x 3 + 24 x 4 layers); smaller inputs: the
        # modules whose smallest map stays >= wino4_min_hw
        assert sum(1 for o in plan.ops if o['group'] > 1) == (64 if size == 224 else 8)
    finally:
        bb.group_branches, bb.multi_stream, bb.use_graph, bb.conv_algo, bb.wino4_min_hw = keep
        bb.wino4_ksplit = keep_split
    assert torch.equal(again, got)
    assert (got - ref).abs().max().item() <= 2e-5 * max(1.0, ref.abs().max().item())
    assert (split - ref).abs().max().item() <= 2e-5 * max(1.0, ref.abs().max().item())
    if size == 224:
        assert not torch.equal(split, ref)               # the split layers really ran


@pytest.mark.parametrize('wino', [True, 4])
@pytest.mark.parametrize('kind', ['mean3', 'scale100', 'relu_like'])
def test_winograd_kernels_on_shifted_and_scaled_inputs(wino, kind):
    """the F(4x4) points {0, +-1, +-2, inf} amplify DC, and the kernel tests only used
    zero-mean unit-variance operands.  Inputs with a +3 sigma mean, with scale 100, and post-ReLU-like
    (non-negative, mean ~0.9 sigma): error against float64 RELATIVE TO THE OUTPUT SCALE."""
    _need_gpu()
    from shapy_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(7)
    worst = 0.0
    for (B, H, W, C, O) in ((2, 56, 56, 48, 48), (2, 28, 28, 96, 96), (2, 14, 14, 192, 192), (4, 7, 7, 384, 384)):
        x = torch.randn(B, H, W, C, generator=g)
        x = {'mean3': x + 3.0, 'scale100': 100.0 * x, 'relu_like': torch.relu(x + 0.5)}[kind].cuda()
        w = (torch.randn(O, 3, 3, C, generator=g) / np.sqrt(9 * C)).cuda()
        b = torch.randn(O, generator=g).cuda()
        r = torch.randn(B, H, W, O, generator=g).cuda()
        y = _conv_call(lib, x, w, b, r, True, 1, 1, wino=wino)
        ref = _conv_ref(x, w, b, r, True, 1, 1)
        err = (y.cpu().double() - ref).abs().max().item() / ref.abs().max().item()
        worst = max(worst, err)
        # measured on MI355X: F(2x2) <= 9e-7, F(4x4) <= 4e-6 of the output scale on all three kinds
        assert err < (2e-5 if wino == 4 else 5e-6), (kind, (B, H, W, C, O), err)
    print(f'winograd F({"4x4" if wino == 4 else "2x2"}) {kind}: worst error / output scale {worst:.2e}')


def test_winograd_guard_calibration_and_wide_batchnorm_scales():
    """The Winograd numerics guard (HighResolutionNet.calibrate, run on the first batch after the
    weights changed): (1) benign synthetic weights -> every Winograd layer is far inside the budget,
    nothing is demoted; (2) "wild" weights -- BatchNorm gamma / sigma spread over 10^3 per channel,
    positive post-ReLU means -- with conv_algo left at its default still meet 1e-4 on the features
    against the CPU oracle; (3) with an artificially small budget the worst layers ARE demoted
    (F(4x4) -> F(2x2) -> direct), logged, and the rebuilt plan carries the demotions."""
    _need_gpu()
    import sys
    sys.path.insert(0, osp.join(osp.dirname(osp.dirname(osp.abspath(__file__))), 'tools'))
    import __graft_entry__ as ge
    from oracle import hrnet_torch
    from shapy_amd.utils import synthetic as syn
    from wino_guard_report import make_wild
    net, _ = ge.make_network()
    bb = net.backbone
    assert bb.wino_guard and bb.conv_algo == 'winograd4'
    x = torch.from_numpy(syn.synthetic_images(2, 224, 21)).cuda()
    with torch.no_grad():
        bb(x)
    rep = bb.calibration_report
    assert rep is not None and len(rep['layers']) > 200 and rep['demoted'] == {}
    assert max(l[2] for l in rep['layers']) < 0.25 * bb.wino_budget          # measured: 1.3e-6
    # (2) wide BatchNorm scales
    make_wild(bb)
    with torch.no_grad():
        feat = bb(x)['concat'].cpu()
    assert bb.calibration_report is not rep                                    # re-calibrated
    sd = {'backbone.' + k: v.detach().cpu() for k, v in bb.state_dict().items()}
    torch.set_num_threads(min(torch.get_num_threads(), 32))
    with torch.no_grad():
        ref = hrnet_torch.hrnet_forward(sd, x.cpu(), prefix='backbone.')
    scale = ref.abs().max().item()
    err = (feat - ref).abs().max().item()
    print(f'wild weights: feature scale {scale:.3g}, error vs CPU oracle {err:.2e}, demoted {bb.calibration_report["demoted"]}')
    assert 5.0 < scale < 1e3 and err < 1e-4
    # (3) the mechanism: a budget below the F(4x4) layers' benign error demotes the worst of them
    msgs = []
    rep3 = bb.calibrate(x, budget=6e-7, log=msgs.append)
    assert rep3['demoted'] and len(msgs) >= len(rep3['demoted'])
    assert all(v in ('winograd', 'direct') for v in rep3['demoted'].values())
    eng = bb._compile(224, 224, x.device)
    for o in eng['plan'].ops:
        to = rep3['demoted'].get(o.get('name'))
        if to == 'direct':
            assert o['wino_off'] < 0
        elif to == 'winograd':
            assert o['wino_off'] >= 0 and not (o['tile'] & 0x100000)
    with torch.no_grad():
        feat3 = bb(x)['concat'].cpu()
    assert (feat3 - ref).abs().max().item() < 1e-4


@pytest.mark.parametrize('B,size,graph', [(3, 96, False), (64, 224, False), (2, 224, True), (2, 256, False)])
def test_hrnet_event_driven_plan_equals_barrier_plan(network, B, size, graph):
    """dag (default): dependency events between the lanes instead of a join between the branches and
    the fuse layers of every module, fuse chains on auxiliary streams -- the same launches on the
    same (differently packed) buffers: bit-identical features, three forwards in a row (the events
    are reused), eager and captured."""
    from shapy_amd.utils import synthetic as syn
    from shapy_amd.models.backbone import hrnet as hrnet_mod
    bb = network.backbone
    keep = bb.dag, bb.multi_stream, bb.use_graph
    x = torch.from_numpy(syn.synthetic_images(B, size, 12)).cuda()
    try:
        bb.multi_stream, bb.use_graph = True, graph
        if size == 256:      # the reference's default crop size under the product's default algorithm
            bb.conv_algo = hrnet_mod.DEFAULT_CONV_ALGO
        bb.dag = False
        with torch.no_grad():
            ref = bb(x)['concat'].clone()
        bb.dag = True
        with torch.no_grad():
            got = [bb(x)['concat'].clone() for _ in range(3)]
        torch.cuda.synchronize()
        if not graph:        # (captured plans keep the barrier form)
            plan = [e for k, e in bb._engine.items()
                    if k[7] is False and k[8] is True and k[0] == size][-1]['plan']      # not grouped, dag
            assert sum(1 for o in plan.ops if o['sig'] >= 0) > 20
    finally:
        bb.dag, bb.multi_stream, bb.use_graph = keep
        bb.conv_algo = 'direct'
    assert all(torch.equal(g, ref) for g in got)


@pytest.mark.parametrize('B,size,cdt', [(3, 96, 'f32'), (12, 96, 'f32'), (64, 224, 'f32'), (12, 96, 'bf16')])
def test_hrnet_prefetched_prologue_bit_identical(network, B, size, cdt):
    """forward(x, prefetch=next_x): the next batch's stem + layer1 on a side stream in a second workspace
    (backbone/prefetch.py).  Same kernels in the same order per image -> the features of a pipelined loop over
    alternating inputs equal the plain forwards bit for bit; B <= 16 issues the prologue before the rest, larger
    batches behind it.  A stash that does not match the next call (another tensor, an in-place edit) is ignored."""
    from shapy_amd.models.backbone import hrnet as hrnet_mod
    from shapy_amd.utils import synthetic as syn
    bb = network.backbone
    keep = bb.multi_stream, bb.compute_dtype
    bb.multi_stream, bb.conv_algo, bb.compute_dtype = True, hrnet_mod.DEFAULT_CONV_ALGO, cdt
    xs = [torch.from_numpy(syn.synthetic_images(B, size, 60 + i)).cuda() for i in range(3)]
    try:
        with torch.no_grad():
            refs = [bb(x)['concat'].clone() for x in xs]
            used0, issued0 = bb._prefetch.used, bb._prefetch.issued
            got = []
            for k in range(7):
                got.append(bb(xs[k % 3], prefetch=xs[(k + 1) % 3])['concat'].clone())
            assert bb._prefetch.issued - issued0 == 7 and bb._prefetch.used - used0 == 6
            for k in range(7):
                assert torch.equal(got[k], refs[k % 3]), k
            # the stash (xs[1]) is not what comes next: full forward, right answer; the stash is dropped
            assert torch.equal(bb(xs[2])['concat'], refs[2]) and bb._prefetch.pending is None
            # an in-place edit between prefetch and use: the version counter differs -> full forward on the new data
            y = xs[0].clone()
            bb(xs[1], prefetch=y)
            y.mul_(0.5)
            used1 = bb._prefetch.used
            edited = bb(y)['concat'].clone()
            assert bb._prefetch.used == used1
            assert torch.equal(edited, bb(y.clone())['concat'])
            # a view of the same memory is the same input
            bb(xs[1], prefetch=xs[0])
            assert torch.equal(bb(xs[0][:])['concat'], refs[0]) and bb._prefetch.used == used1 + 1
            # single-stream forwards and shapes that do not match ignore the argument
            bb.multi_stream = False
            issued1 = bb._prefetch.issued
            assert torch.equal(bb(xs[0], prefetch=xs[1])['concat'], bb(xs[0])['concat'])
            bb.multi_stream = True
            assert torch.equal(bb(xs[0], prefetch=xs[1][:1])['concat'], refs[0]) and bb._prefetch.issued == issued1
        torch.cuda.synchronize()
    finally:
        bb.multi_stream, bb.compute_dtype = keep
        bb.conv_algo = 'direct'


def test_full_forward_next_images_bit_identical(network):
    """SMPLXRegressor.forward(images, next_images=...): every output of a pipelined loop equals the plain call's."""
    from shapy_amd.models.backbone import hrnet as hrnet_mod
    from shapy_amd.utils import synthetic as syn
    bb = network.backbone
    keep = bb.multi_stream
    bb.multi_stream, bb.conv_algo = True, hrnet_mod.DEFAULT_CONV_ALGO
    xs = [torch.from_numpy(syn.synthetic_images(16, 224, 70 + i)).cuda() for i in range(2)]
    try:
        with torch.no_grad():
            refs = [network(x, None) for x in xs]
            used0 = bb._prefetch.used
            for k in range(4):
                out = network(xs[k & 1], None, next_images=xs[(k + 1) & 1])
                ref = refs[k & 1]
                assert torch.equal(out['features'], ref['features'])
                assert torch.equal(out['stage_02']['betas'], ref['stage_02']['betas'])
                assert torch.equal(out['stage_02']['vertices'], ref['stage_02']['vertices'])
            assert bb._prefetch.used - used0 == 3
        torch.cuda.synchronize()
    finally:
        bb.multi_stream = keep
        bb.conv_algo = 'direct'


@pytest.mark.parametrize('B', [32, 16])
def test_full_forward_mid_batch_buckets_with_next_images_vs_oracle(network, B):
    """The batch buckets between the reference goldens (B <= 4) and the headline (B = 64): B = 32 (split-K policy
    {(384,4): 4, (192,16): 2} + implicit-GEMM splits; stem + layer1 of the next batch behind the rest) and B = 16
    (same plan bucket, EARLY prologue: stem + layer1 + stage 2 issued in front of the running batch) -- the plans
    configs[2]'s per-GPU shard and evaluate.py's batches take.  f32, default algorithm, @224, in a pipelined loop
    (next_images), every output of the SECOND step (whose prologue ran under the first) against the CPU oracle
    at 1e-4 (iterative_regressor.py:623-870)."""
    import __graft_entry__ as ge
    from shapy_amd.models.backbone import hrnet as hrnet_mod
    from shapy_amd.utils import synthetic as syn
    bb = network.backbone
    keep = (bb.multi_stream, bb.compute_dtype, bb.conv_algo)
    bb.multi_stream, bb.compute_dtype, bb.conv_algo = True, 'f32', hrnet_mod.DEFAULT_CONV_ALGO
    xs_np = [syn.synthetic_images(B, 224, 300 + B + i) for i in range(2)]
    xs = [torch.from_numpy(a).cuda() for a in xs_np]
    try:
        with torch.no_grad():
            used0 = bb._prefetch.used
            network(xs[0], None, next_images=xs[1])
            out = network(xs[1], None, next_images=xs[0])
            assert bb._prefetch.used - used0 == 1, 'the second step did not run on the prefetched prologue'
            bb.drop_prefetch()
        torch.cuda.synchronize()
    finally:
        bb.multi_stream, bb.compute_dtype, bb.conv_algo = keep
    ref = ge.oracle_forward(xs_np[1])
    st, rs = out['stage_02'], ref['stages'][-1]
    errs = {
        'features': np.abs(out['features'].cpu().numpy() - ref['features']).max(),
        'betas': np.abs(st['betas'].cpu().numpy() - rs['betas']).max(),
        'vertices': np.abs(st['vertices'].cpu().numpy() - rs['vertices']).max(),
        'joints': np.abs(st['joints']._t.cpu().numpy() - rs['joints']).max(),
    }
    for k in ('mass', 'height', 'chest', 'waist', 'hips'):
        errs['meas_' + k] = np.abs(out['measurements'][k].cpu().numpy() - ref['measurements'][k]).max()
    for k, v in errs.items():
        print(f'B={B} pipelined {k:14s} {v:.3e}')
    bad = {k: v for k, v in errs.items() if not v < 1e-4}
    assert not bad, bad


def test_hrnet_prefetch_stash_rules(network):
    """What makes a stashed prologue stale (prefetch.py): an in-place torch write bumps the version counter ->
    ignored; a write BEHIND torch's back (here: through a DLPack alias, which has a version counter of its own)
    is invisible -> the documented rule is drop_prefetch() before such a write, after which the forward runs in
    full; tensors created under inference_mode have no version counter -> never stashed, no exception."""
    from torch.utils import dlpack
    from shapy_amd.models.backbone import hrnet as hrnet_mod
    from shapy_amd.utils import synthetic as syn
    bb = network.backbone
    keep = (bb.multi_stream, bb.compute_dtype, bb.conv_algo)
    bb.multi_stream, bb.compute_dtype, bb.conv_algo = True, 'f32', hrnet_mod.DEFAULT_CONV_ALGO
    a = torch.from_numpy(syn.synthetic_images(4, 96, 11)).cuda()
    b = torch.from_numpy(syn.synthetic_images(4, 96, 12)).cuda()
    try:
        with torch.no_grad():
            plain = lambda t: bb(t.clone())['concat'].clone()
            # (1) in-place torch write: recognised
            used = bb._prefetch.used
            bb(a, prefetch=b)
            b.mul_(0.5)
            out = bb(b)['concat'].clone()
            assert bb._prefetch.used == used and torch.equal(out, plain(b))
            # (2) write through an alias torch does not track + drop_prefetch(): full forward, right answer
            bb(a, prefetch=b)
            alias = dlpack.from_dlpack(dlpack.to_dlpack(b))
            bb.drop_prefetch()
            alias.add_(0.25)
            torch.cuda.synchronize()
            out = bb(b)['concat'].clone()
            assert bb._prefetch.used == used and torch.equal(out, plain(b))
            # (3) untouched: the stash is used and bit-identical
            bb(a, prefetch=b)
            out = bb(b)['concat'].clone()
            assert bb._prefetch.used == used + 1 and torch.equal(out, plain(b))
        # (4) inference tensors: no version counter; forward works, nothing is stashed
        with torch.inference_mode():
            ai, bi = a.clone(), b.clone()
            issued = bb._prefetch.issued
            o1 = bb(ai, prefetch=bi)['concat'].clone()
            o2 = bb(bi)['concat'].clone()
            assert bb._prefetch.issued == issued
        with torch.no_grad():
            assert torch.equal(o1, plain(a)) and torch.equal(o2, plain(b))
        torch.cuda.synchronize()
    finally:
        bb.drop_prefetch()
        bb.multi_stream, bb.compute_dtype, bb.conv_algo = keep


def test_hrnet_head_gemms_on_bf16x6_vs_f32_kernel(network):
    """Opt-in (x6_gemm_min_batch = 64): the head's fifteen wide 1x1 GEMMs on the bf16 matrix cores
    (SHAPY_TILE_X6 in a float32 plan: float32 tensors, exact 3-way bf16 split, f32 accumulate).  Against the
    all-f32-MFMA plan of the same batch the features move by float32 rounding only."""
    from shapy_amd import _lib
    from shapy_amd.models.backbone import hrnet as hrnet_mod
    from shapy_amd.utils import synthetic as syn
    bb = network.backbone
    keep = bb.multi_stream, bb.x6_gemm_min_batch
    bb.multi_stream, bb.conv_algo = True, hrnet_mod.DEFAULT_CONV_ALGO
    x = torch.from_numpy(syn.synthetic_images(64, 224, 77)).cuda()
    try:
        with torch.no_grad():
            bb.x6_gemm_min_batch = 0
            f32 = bb(x)['concat'].clone()
            bb.x6_gemm_min_batch = 64
            mixed = bb(x)['concat'].clone()
            small = bb(x[:8])['concat'].clone()            # a smaller batch keeps the f32 kernel ...
            bb.x6_gemm_min_batch = 0
            assert torch.equal(small, bb(x[:8])['concat'])  # ... bit for bit
        plans = [e['plan'] for k, e in bb._engine.items() if k[0] == 224 and k[12] is True]
        assert plans and sum(1 for o in plans[-1].ops if o['tile'] & _lib.TILE_X6) == 15
    finally:
        bb.multi_stream, bb.x6_gemm_min_batch = keep
        bb.conv_algo = 'direct'
    scale = f32.abs().max().item()
    err = (mixed - f32).abs().max().item()
    assert 0 < err < 2e-5 * max(1.0, scale), (err, scale)


def test_hrnet_two_host_threads_on_two_streams_bit_identical(network):
    """Two host threads issue forwards concurrently, each on its own stream: the executor serialises
    the ENQUEUE of a forward (one process-wide lock around the whole issue incl. its event records /
    waits on the shared side streams), every caller stream has its own workspace -- results equal the
    single-threaded ones bit for bit."""
    import threading
    from shapy_amd.models.backbone import hrnet as hrnet_mod
    from shapy_amd.utils import synthetic as syn
    bb = network.backbone
    keep = bb.multi_stream
    bb.multi_stream, bb.conv_algo = True, hrnet_mod.DEFAULT_CONV_ALGO
    xs = [torch.from_numpy(syn.synthetic_images(3, 96, 40 + i)).cuda() for i in range(2)]
    try:
        with torch.no_grad():
            refs = [bb(x)['concat'].clone() for x in xs]
        torch.cuda.synchronize()
        outs, errs = [None, None], []

        def work(i):
            try:
                st = torch.cuda.Stream()
                with torch.cuda.stream(st), torch.no_grad():
                    got = [bb(xs[i])['concat'].clone() for _ in range(6)]
                st.synchronize()
                outs[i] = got
            except Exception as e:               # noqa: BLE001
                errs.append(e)
        ts = [threading.Thread(target=work, args=(i,)) for i in range(2)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert not errs, errs
    finally:
        bb.multi_stream, bb.conv_algo = keep, 'direct'
    for i in range(2):
        assert all(torch.equal(g, refs[i]) for g in outs[i])


def test_conv2d_group_c_abi_matches_single_launches():
    """shapy_conv2d_group through the C-ABI: groups of 1-4 layers incl. partly filled workgroups,
    a channel-offset epilogue, Cout = 144 (the generic XCD split), more tasks than workgroup slots;
    refusals leave the outputs untouched."""
    _need_gpu()
    import subprocess
    import sys
    root = osp.dirname(osp.dirname(osp.abspath(__file__)))
    r = subprocess.run([sys.executable, osp.join(root, 'tools', 'wino4g_check.py'), '--canary'],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and 'CANARY OK' in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    from shapy_amd import _lib
    lib = _lib.load()
    # a layer that is not an F(4x4) layer -> SHAPY_EINVAL, nothing launched
    x = torch.randn(1, 8, 8, 16).cuda()
    w = torch.randn(48, 3, 3, 16).cuda()
    out = torch.full((1, 8, 8, 48), 7.0).cuda()
    d = _lib.ShapyConv()
    d.dtype = _lib.DTYPE_F32
    d.in_ = x.data_ptr(); d.wgt = w.data_ptr(); d.out = out.data_ptr()
    d.B, d.Hi, d.Wi, d.Cin, d.in_ld = 1, 8, 8, 16, 16
    d.Ho, d.Wo, d.Cout = 8, 8, 48
    d.ksize, d.stride, d.pad, d.out_ld, d.ups = 3, 1, 1, 48, 1
    arr = (_lib.ShapyConv * 1)(d)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.shapy_conv2d_group(arr, 1, stream) == -1
    assert lib.shapy_conv2d_group(arr, 5, stream) == -1
    torch.cuda.synchronize()
    assert (out == 7.0).all()


@pytest.mark.parametrize('tag,b,s', [('b2_64', 2, 64), ('b1_224', 1, 224)])
def test_hrnet_bf16_features_vs_f32_golden(network, golden_dir, tag, b, s):
    """BASELINE configs[2]: bf16 weights/activations, f32 accumulate.  It does not meet the 1e-4
    bar (that is the f32 path's job); its error is reported and bounded separately."""
    from shapy_amd.utils import synthetic as syn
    g = np.load(osp.join(golden_dir, 'hrnet_golden.npz'))
    x = torch.from_numpy(syn.synthetic_images(b, s, 0)).cuda()
    network.backbone.compute_dtype = 'bf16'
    try:
        with torch.no_grad():
            feat = network.backbone(x)['concat']
        torch.cuda.synchronize()
    finally:
        network.backbone.compute_dtype = 'f32'
    ref = g[tag]
    err = np.abs(feat.cpu().numpy() - ref)
    rel = err.max() / np.abs(ref).max()
    print(tag, 'bf16 max abs err', err.max(), 'mean abs err', err.mean(), 'rel to max', rel)
    assert rel < 0.05, rel


@pytest.mark.parametrize('cdt', ['f32', 'f32x6'])
def test_full_forward_vs_reference_golden(network, golden_dir, cdt):
    from shapy_amd.utils import synthetic as syn
    g = np.load(osp.join(golden_dir, 'regressor_golden.npz'))
    x = torch.from_numpy(syn.synthetic_images(4, 224, 0)).cuda()
    network.backbone.multi_stream = True
    network.backbone.compute_dtype = cdt
    try:
        with torch.no_grad():
            out = network(x, None)
        torch.cuda.synchronize()
    finally:
        network.backbone.compute_dtype = 'f32'
    assert sorted(str(k) for k in out.keys()) == list(g['out_keys'])
    st = out['stage_02']
    assert sorted(st.keys()) == list(g['stage_keys'])
    errs = {}
    errs['features'] = np.abs(out['features'].cpu().numpy() - g['features']).max()
    for i in range(3):
        s = out[f'stage_{i:02d}']
        for k in ('betas', 'raw_body_pose', 'raw_global_rot', 'camera'):
            errs[f'stage{i}_{k}'] = np.abs(s[k].cpu().numpy() - g[f'stage{i}_{k}']).max()
    errs['global_rot'] = np.abs(st['global_rot'].cpu().numpy() - g['global_rot']).max()
    errs['body_pose'] = np.abs(st['body_pose'].cpu().numpy() - g['body_pose']).max()
    errs['joints'] = np.abs(st['joints']._t.cpu().numpy() - g['joints']).max()
    errs['vertices'] = np.abs(st['vertices'].cpu().numpy()[:, ::SUB] - g['vertices_sub']).max()
    errs['v_shaped'] = np.abs(st['v_shaped'].cpu().numpy()[:, ::SUB] - g['v_shaped_sub']).max()
    pj = out['proj_joints']
    pj = pj._t if hasattr(pj, '_t') else pj
    errs['proj_joints'] = np.abs(pj.cpu().numpy() - g['proj_joints']).max()
    errs['cam_scale'] = np.abs(out['camera_parameters'].scale.cpu().numpy() - g['cam_scale']).max()
    for k in ('mass', 'height', 'chest', 'waist', 'hips'):
        errs['meas_' + k] = np.abs(out['measurements'][k].cpu().numpy() - g['meas_' + k]).max()
    for k, v in errs.items():
        print(f'{k:24s} {v:.3e}')
    assert st['faces'].shape == (20908, 3)
    bad = {k: v for k, v in errs.items() if not v < 1e-4}
    assert not bad, bad


@pytest.mark.parametrize('algo,multi_stream,group', [
    ('direct', True, False), ('winograd', True, False), ('winograd4', True, False),
    ('winograd4', False, True), ('winograd4', True, True)])
def test_hrnet_features_256_vs_reference_golden(network, golden_dir, algo, multi_stream, group):
    """The reference's DEFAULT crop size, 256 x 256 (config/datasets_defaults.py:30; neither YAML
    overrides it) -- the size demo.py feeds the network: 64 / 32 / 16 / 8-pixel maps, i.e. other
    F(4x4) tile counts, LPT schedules and workspace packings than 56 / 28 / 14 / 7.  Every float32
    algorithm (and the grouped persistent launches) against the REAL reference's CPU features
    (tests/golden/make_golden_256.py) at 1e-4."""
    from shapy_amd import _lib
    from shapy_amd.utils import synthetic as syn
    g = np.load(osp.join(golden_dir, 'hrnet_golden_256.npz'))
    x = torch.from_numpy(syn.synthetic_images(2, 256, 0)).cuda()
    bb = network.backbone
    keep = bb.multi_stream, bb.group_branches
    bb.multi_stream, bb.group_branches, bb.conv_algo = multi_stream, group, algo
    try:
        with torch.no_grad():
            feat = bb(x)['concat']
        torch.cuda.synchronize()
        eng = [e for k, e in bb._engine.items() if k[4] == algo and k[0] == 256][-1]
        n4 = sum(1 for o in eng['plan'].ops if o['tile'] & _lib.TILE_WINO4)
        ng = sum(1 for o in eng['plan'].ops if o['group'] > 1)
    finally:
        bb.conv_algo = 'direct'
        bb.multi_stream, bb.group_branches = keep
    err = np.abs(feat.cpu().numpy() - g['b2_256']).max()
    print('256x256', algo, 'multi_stream', multi_stream, 'group', group, 'F(4x4) layers', n4,
          'launch groups', ng, 'max abs err', err)
    assert (n4 >= 200) == (algo == 'winograd4')
    assert (ng > 0) == bool(group)
    assert err < 1e-4, err


def test_full_forward_256_vs_reference_golden(network, golden_dir):
    """Whole hot path at the reference's default crop size under the product's default algorithm
    (F(4x4) from 7-pixel maps -- here 8) against the real reference's SMPLXRegressor.forward."""
    from shapy_amd.models.backbone import hrnet as hrnet_mod
    from shapy_amd.utils import synthetic as syn
    g = np.load(osp.join(golden_dir, 'regressor_golden_256.npz'))
    x = torch.from_numpy(syn.synthetic_images(2, 256, 0)).cuda()
    network.backbone.multi_stream = True
    network.backbone.conv_algo = hrnet_mod.DEFAULT_CONV_ALGO
    try:
        with torch.no_grad():
            out = network(x, None)
        torch.cuda.synchronize()
    finally:
        network.backbone.conv_algo = 'direct'
    st = out['stage_02']
    errs = {'features': np.abs(out['features'].cpu().numpy() - g['features']).max()}
    for i in range(3):
        s = out[f'stage_{i:02d}']
        for k in ('betas', 'raw_body_pose', 'raw_global_rot', 'camera'):
            errs[f'stage{i}_{k}'] = np.abs(s[k].cpu().numpy() - g[f'stage{i}_{k}']).max()
    errs['joints'] = np.abs(st['joints']._t.cpu().numpy() - g['joints']).max()
    errs['vertices'] = np.abs(st['vertices'].cpu().numpy()[:, ::SUB] - g['vertices_sub']).max()
    errs['v_shaped'] = np.abs(st['v_shaped'].cpu().numpy()[:, ::SUB] - g['v_shaped_sub']).max()
    pj = out['proj_joints']
    pj = pj._t if hasattr(pj, '_t') else pj
    errs['proj_joints'] = np.abs(pj.cpu().numpy() - g['proj_joints']).max()
    for k in ('mass', 'height', 'chest', 'waist', 'hips'):
        errs['meas_' + k] = np.abs(out['measurements'][k].cpu().numpy() - g['meas_' + k]).max()
    for k, v in errs.items():
        print(f'{k:24s} {v:.3e}')
    bad = {k: v for k, v in errs.items() if not v < 1e-4}
    assert not bad, bad


def test_smplx_ops_vs_reference_golden(network, golden_dir):
    g = np.load(osp.join(golden_dir, 'ops_golden.npz'))
    from shapy_amd.models.common.pose_utils import AADecoder, ContinuousRotReprDecoder
    aa = torch.from_numpy(g['rodrigues_in']).cuda()
    R = AADecoder(aa.shape[0])(aa.reshape(1, -1))[0]
    assert np.abs(R.cpu().numpy() - g['rodrigues_out']).max() < 1e-5
    x6 = torch.from_numpy(g['cont6d_in']).cuda()
    R6 = ContinuousRotReprDecoder(22).cuda()(x6)
    assert np.abs(R6.cpu().numpy() - g['cont6d_out']).max() < 1e-5
    rot = ContinuousRotReprDecoder(22).cuda()(torch.from_numpy(g['smplx_pose6d']).cuda())
    with torch.no_grad():
        so = network.model(global_rot=rot[:, :1], body_pose=rot[:, 1:],
                           betas=torch.from_numpy(g['smplx_betas']).cuda(),
                           get_skin=True, return_shaped=True)
    torch.cuda.synchronize()
    ej = np.abs(so['joints']._t.cpu().numpy() - g['smplx_joints']).max()
    ev = np.abs(so['vertices'].cpu().numpy()[:, ::SUB] - g['smplx_vertices_sub']).max()
    es = np.abs(so['v_shaped'].cpu().numpy()[:, ::SUB] - g['smplx_v_shaped_sub']).max()
    print('smplx joints', ej, 'vertices', ev, 'v_shaped', es)
    assert ej < 1e-4 and ev < 1e-4 and es < 1e-5
    cam = torch.from_numpy(g['cam_in']).cuda()
    scale = torch.nn.functional.softplus(cam[:, :1])
    proj = network.projection(so['joints'], scale=scale, translation=cam[:, 1:3])
    assert np.abs(proj._t.cpu().numpy() - g['cam_proj']).max() < 1e-4


@pytest.mark.parametrize('B', [1, 3, 4])
def test_smplx_forward_odd_batches_and_full_pose_vs_oracle(network, B):
    """SMPLX.forward through its generic argument path (not the regressor's fast head) at batch sizes
    whose pose block is not a multiple of 16 bytes: global_rot + body_pose (22 joints: B * 198 floats) and
    all 55 joints given explicitly (identity jaw / eyes / hands) -- the coefficient rows are the GEMM's A
    operand and must stay 16-byte aligned whatever B is.  Also a [1, 10] betas row broadcast to B."""
    from oracle import body_np
    from shapy_amd.utils import synthetic as syn
    model = syn.make_synthetic_smplx(0)
    rng = np.random.default_rng(40 + B)
    rot = body_np.cont_rot_repr_decode(rng.standard_normal((B, 22, 6)).astype(np.float32) * 0.5 +
                                       np.array([1, 0, 0, 1, 0, 0], np.float32)).astype(np.float32)
    betas = (rng.standard_normal((B, 10)) * 1.5).astype(np.float32)
    ref = body_np.smplx_forward(model, rot[:, :1], rot[:, 1:], betas)
    r = torch.from_numpy(rot).cuda()
    bt = torch.from_numpy(betas).cuda()

    def eye(n):
        return torch.eye(3, device='cuda').view(1, 1, 3, 3).expand(B, n, 3, 3).contiguous()
    with torch.no_grad():
        a = network.model(global_rot=r[:, :1], body_pose=r[:, 1:], betas=bt, get_skin=True, return_shaped=True)
        b = network.model(global_rot=r[:, :1], body_pose=r[:, 1:], jaw_pose=eye(1), leye_pose=eye(1),
                          reye_pose=eye(1), left_hand_pose=eye(15), right_hand_pose=eye(15), betas=bt,
                          get_skin=True, return_shaped=True, return_full_pose=True)
        c = network.model(global_rot=r[:, :1], body_pose=r[:, 1:], betas=bt[:1], get_skin=True)
        # parts whose leading dimension is not the batch: the reference views them as reshape(-1, n, 3, 3)
        d = network.model(global_rot=r[:, :1].reshape(B, 3, 3), body_pose=r[:, 1:].reshape(B * 21, 3, 3), betas=bt,
                          get_skin=True, return_shaped=True)
    torch.cuda.synchronize()
    assert torch.equal(a['vertices'], d['vertices']) and torch.equal(a['joints']._t, d['joints']._t)
    for out in (a, b):
        assert np.abs(out['vertices'].cpu().numpy() - ref['vertices']).max() < 1e-4
        assert np.abs(out['joints']._t.cpu().numpy() - ref['joints']).max() < 1e-4
        assert np.abs(out['v_shaped'].cpu().numpy() - ref['v_shaped']).max() < 1e-5
    assert torch.equal(a['vertices'], b['vertices'])
    assert np.abs(b['full_pose'].cpu().numpy() - ref['full_pose']).max() < 1e-6
    ref1 = body_np.smplx_forward(model, rot[:, :1], rot[:, 1:], np.repeat(betas[:1], B, 0))
    assert np.abs(c['vertices'].cpu().numpy() - ref1['vertices']).max() < 1e-4


def test_shipped_sample_pins(network, golden_dir):
    """The reference's shipped SHAPY_A output (img_00.npz): decoder, camera, measurements."""
    g = np.load(osp.join(golden_dir, 'img_00_pins.npz'))
    from shapy_amd.models.common.pose_utils import ContinuousRotReprDecoder
    from shapy_amd.utils import synthetic as syn
    dec = ContinuousRotReprDecoder(21).cuda()
    bp = dec(torch.from_numpy(g['raw_body_pose'][None]).cuda())[0].cpu().numpy()
    gr = ContinuousRotReprDecoder(1).cuda()(torch.from_numpy(g['raw_global_rot'][None]).cuda())[0].cpu().numpy()
    assert np.abs(bp - g['body_pose']).max() < 1e-6 and np.abs(gr - g['global_rot']).max() < 1e-6
    cam = torch.from_numpy(g['camera'][None]).cuda()
    proj = network.projection(torch.from_numpy(g['joints'][None]).cuda(),
                              scale=torch.nn.functional.softplus(cam[:, :1]), translation=cam[:, 1:3])
    assert np.abs(proj.cpu().numpy()[0] - g['proj_joints']).max() < 1e-5
    faces, meshes = syn.load_topology()
    out = network.body_measurements.forward_vertices(
        torch.from_numpy(meshes).cuda(), torch.from_numpy(faces).cuda())
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    print('measurements (mesh 0):', out[0])
    assert int(network.body_measurements.last_overflow.item()) == 0
    for i, k in enumerate(('mass', 'height', 'chest', 'waist', 'hips')):
        tol = 1e-4 if k == 'mass' else 2e-6
        assert abs(out[0, i] - float(g['meas_' + k][0])) < tol, (k, out[0, i], g['meas_' + k])
    mg = np.load(osp.join(golden_dir, 'measure_golden.npz'))
    for i, k in enumerate(('mass', 'height', 'chest', 'waist', 'hips')):
        np.testing.assert_allclose(out[:, i], mg[k], rtol=3e-6, atol=2e-6, err_msg=k)
    # the reference's [B,F,3,3] triangle signature gives the same numbers
    tris = torch.from_numpy(np.ascontiguousarray(meshes[:, faces])).cuda()
    m2 = network.body_measurements(tris)['measurements']
    for i, k in enumerate(('mass', 'height', 'chest', 'waist', 'hips')):
        assert np.array_equal(m2[k]['tensor'].cpu().numpy(), out[:, i]), k


def test_mesh_to_mesh_operator_bit_exact_vs_oracle():
    _need_gpu()
    import mesh_mesh_intersect_cuda
    from oracle import measure as om
    from shapy_amd.utils import synthetic as syn
    faces, meshes = syn.load_topology()
    tris = np.ascontiguousarray(meshes[:, faces])                       # 4,F,3,3
    heights = np.array([-0.0343, -0.2515, -0.4845, 0.2], np.float32)
    q = om.plane_triangles(heights)
    # a few arbitrary query triangles as well (sliced from another mesh)
    q2 = np.ascontiguousarray(np.concatenate([q, tris[::-1][:, 5000:5006]], axis=1))
    for query, mc in ((q, 256), (q2, 64), (q, 16)):
        f_ref, b_ref = om.mesh_to_mesh_forward(query, tris, mc)
        f, b = mesh_mesh_intersect_cuda.mesh_to_mesh_forward(
            torch.from_numpy(query).cuda(), torch.from_numpy(tris).cuda(), max_collisions=mc)
        torch.cuda.synchronize()
        assert f.dtype == torch.int64 and f.shape == (4, query.shape[1] * mc)
        assert b.shape == (4, query.shape[1] * mc, 2, 3)
        assert np.array_equal(f.cpu().numpy(), f_ref)
        assert np.array_equal(b.cpu().numpy(), b_ref)
        ov = int(mesh_mesh_intersect_cuda.mesh_to_mesh_forward.last_overflow.item())
        assert ov == om.mesh_to_mesh_forward.last_dropped
    # empty / ragged edge cases
    e = mesh_mesh_intersect_cuda.mesh_to_mesh_forward(
        torch.zeros(1, 2, 3, 3).cuda(), torch.from_numpy(tris[:1, :0]).cuda(), max_collisions=4)
    assert (e[0] == -1).all() and (e[1] == 0).all()


def test_mesh_to_mesh_operator_float64_bit_exact_vs_oracle():
    """The reference's second instantiation (AT_DISPATCH_FLOATING_TYPES, mesh_mesh_intersect_cuda_op.cu:996):
    float64 triangles through shapy_mesh_to_mesh_f64 -- faces and float64 barycentrics bit-equal to the
    oracle's float64 build (same float constants inside: CMP in float, the 1e-4 cut), plane quads and
    arbitrary query triangles, overflow, mixed dtypes refused."""
    _need_gpu()
    import mesh_mesh_intersect_cuda
    from oracle import measure as om
    from shapy_amd.utils import synthetic as syn
    faces, meshes = syn.load_topology()
    tris = np.ascontiguousarray(meshes[:, faces]).astype(np.float64)    # 4,F,3,3
    tris += 1e-9 * np.random.default_rng(3).standard_normal(tris.shape)  # genuinely float64 coordinates
    q = om.plane_triangles(np.array([-0.0343, -0.2515, -0.4845, 0.2], np.float32)).astype(np.float64)
    q2 = np.ascontiguousarray(np.concatenate([q, tris[::-1][:, 5000:5030]], axis=1))       # Q = 32
    for query, mc in ((q, 256), (q2, 64), (q, 16)):
        f_ref, b_ref = om.mesh_to_mesh_forward_f64(query, tris, mc)
        f, b = mesh_mesh_intersect_cuda.mesh_to_mesh_forward(
            torch.from_numpy(query).cuda(), torch.from_numpy(tris).cuda(), max_collisions=mc)
        torch.cuda.synchronize()
        assert f.dtype == torch.int64 and b.dtype == torch.float64
        assert b.shape == (4, query.shape[1] * mc, 2, 3)
        assert np.array_equal(f.cpu().numpy(), f_ref)
        assert np.array_equal(b.cpu().numpy(), b_ref)
        assert int(mesh_mesh_intersect_cuda.mesh_to_mesh_forward.last_overflow.item()) == \
            om.mesh_to_mesh_forward_f64.last_dropped
        assert (f_ref >= 0).sum() > 100
    # next to the float32 operator on the same (rounded) triangles: the same faces, barycentrics to rounding
    f32 = mesh_mesh_intersect_cuda.mesh_to_mesh_forward(
        torch.from_numpy(q.astype(np.float32)).cuda(), torch.from_numpy(tris.astype(np.float32)).cuda(),
        max_collisions=256)
    f64 = mesh_mesh_intersect_cuda.mesh_to_mesh_forward(
        torch.from_numpy(q).cuda(), torch.from_numpy(tris).cuda(), max_collisions=256)
    same = (f32[0] == f64[0])
    assert same.float().mean().item() > 0.99
    assert (f32[1].double() - f64[1])[same].abs().max().item() < 1e-4
    with pytest.raises(NotImplementedError):
        mesh_mesh_intersect_cuda.mesh_to_mesh_forward(
            torch.from_numpy(q.astype(np.float32)).cuda(), torch.from_numpy(tris).cuda())


def test_mesh_to_mesh_bvh_large_target_fallback_paths_vs_oracle():
    """Targets beyond what the LBVH build keeps in LDS (SMPL-X: sorted keys as (Morton, face16) and
    the refit's ready lists fit 128 KB up to ~21,800 / ~26,000 triangles): two bodies side by side
    = 41,816 triangles take the build's global-memory paths (64-bit keys from L2 for the radix
    tree, climbing refit with workgroup-scope fences, three 16,384-key sort blocks + global merge
    stages).  Same hits as the brute-force C oracle."""
    _need_gpu()
    import mesh_mesh_intersect_cuda
    from oracle import measure as om
    from shapy_amd.utils import synthetic as syn
    faces, meshes = syn.load_topology()
    tris = np.ascontiguousarray(meshes[:, faces])                       # 4,F,3,3
    shift = np.array([0.35, 0.0, 0.0], np.float32)
    target = np.ascontiguousarray(np.concatenate([tris[[0, 1]], tris[[2, 3]] + shift], axis=1))   # 2 x 41,816
    q = np.ascontiguousarray(np.concatenate([tris[[1, 0]][:, 3000:3040], tris[[3, 2]][:, 5000:5040] + shift],
                                            axis=1))                    # 80 query triangles
    mc = 96
    f_ref, b_ref = om.mesh_to_mesh_forward(q, target, mc)
    assert om.mesh_to_mesh_forward.last_dropped == 0 and (f_ref >= 0).sum() > 100
    f, b = mesh_mesh_intersect_cuda.mesh_to_mesh_forward(
        torch.from_numpy(q).cuda(), torch.from_numpy(target).cuda(), max_collisions=mc)
    torch.cuda.synchronize()
    assert int(mesh_mesh_intersect_cuda.mesh_to_mesh_forward.last_overflow.item()) == 0
    assert np.array_equal(f.cpu().numpy(), f_ref)
    assert np.array_equal(b.cpu().numpy(), b_ref)


def test_measurements_large_batch_properties(network):
    """Config 4 at full size (1,000 meshes): size-independent properties."""
    from shapy_amd.utils import synthetic as syn
    faces, meshes = syn.load_topology()
    r = syn.rng_for(0, 'config4')
    w = r.dirichlet(np.ones(4), size=1000).astype(np.float32)
    s = r.uniform(0.9, 1.1, size=1000).astype(np.float32)
    w[0] = [1, 0, 0, 0]; s[0] = 1
    v = torch.from_numpy(np.einsum('nk,kvc->nvc', w, meshes) * s[:, None, None]).cuda()
    f = torch.from_numpy(faces).cuda()
    bm = network.body_measurements
    out = bm.forward_vertices(v, f).cpu().numpy()
    assert int(bm.last_overflow.item()) == 0
    # idempotence / determinism despite atomics
    out2 = bm.forward_vertices(v, f).cpu().numpy()
    assert np.array_equal(out, out2)
    # scaling a mesh by s scales lengths by s and mass by s^3
    out_s = bm.forward_vertices(v * 1.05, f).cpu().numpy()
    np.testing.assert_allclose(out_s[:, 1:], out[:, 1:] * 1.05, rtol=2e-4)
    np.testing.assert_allclose(out_s[:, 0], out[:, 0] * 1.05 ** 3, rtol=2e-4)
    # batch independence: a mesh measured alone gives the same numbers
    for i in (0, 17, 999):
        one = bm.forward_vertices(v[i:i + 1], f).cpu().numpy()
        assert np.array_equal(one[0], out[i])
    assert abs(out[0, 2] - 0.8745367) < 2e-6      # mesh 0 is the shipped sample


def test_mesh_to_mesh_bvh_path_bit_exact_vs_oracle():
    """Large query meshes go through the LBVH (csrc/bvh.hip): same result as the brute-force
    C oracle (and therefore as the scan path)."""
    _need_gpu()
    import mesh_mesh_intersect_cuda
    from oracle import measure as om
    from shapy_amd.utils import synthetic as syn
    faces, meshes = syn.load_topology()
    tris = np.ascontiguousarray(meshes[:, faces])                       # 4,F,3,3
    target = np.ascontiguousarray(tris[[0, 1, 2]])
    # query: 700 triangles of a *different* body (bodies overlap in space) + the plane quad
    q = np.ascontiguousarray(np.concatenate(
        [tris[[1, 2, 3]][:, 3000:3700], om.plane_triangles(np.array([-0.03, -0.25, -0.48], np.float32))],
        axis=1))
    mc = 320
    f_ref, b_ref = om.mesh_to_mesh_forward(q, target, mc)
    assert om.mesh_to_mesh_forward.last_dropped == 0
    assert (f_ref >= 0).sum() > 500
    f, b = mesh_mesh_intersect_cuda.mesh_to_mesh_forward(
        torch.from_numpy(q).cuda(), torch.from_numpy(target).cuda(), max_collisions=mc)
    torch.cuda.synchronize()
    assert int(mesh_mesh_intersect_cuda.mesh_to_mesh_forward.last_overflow.item()) == 0
    assert np.array_equal(f.cpu().numpy(), f_ref)
    assert np.array_equal(b.cpu().numpy(), b_ref)
    # self-intersection query (every triangle at least touches itself and its neighbours)
    sub = np.ascontiguousarray(tris[:2, :1500])
    f_ref, b_ref = om.mesh_to_mesh_forward(sub, sub, 64)
    assert om.mesh_to_mesh_forward.last_dropped == 0
    f, b = mesh_mesh_intersect_cuda.mesh_to_mesh_forward(
        torch.from_numpy(sub).cuda(), torch.from_numpy(sub).cuda(), max_collisions=64)
    torch.cuda.synchronize()
    assert np.array_equal(f.cpu().numpy(), f_ref)
    assert np.array_equal(b.cpu().numpy(), b_ref)


# ------------------------------------------------------------------------------------------
# round 2: the headline configuration at its own size, config 4 mesh by mesh, edge cases
# ------------------------------------------------------------------------------------------
_BS64 = {}


def _oracle_bs64():
    """CPU oracle on the bench's own batch (64 seeded 224x224 images); ~10 s, computed once."""
    if not _BS64:
        import __graft_entry__ as ge
        from shapy_amd.utils import synthetic as syn
        x = syn.synthetic_images(64, 224, 100)
        _BS64['x'] = x
        _BS64['ref'] = ge.oracle_forward(x)
    return _BS64['x'], _BS64['ref']


@pytest.mark.parametrize('cdt', ['f32', 'f32x6', 'f32+winograd', 'f32+winograd4', 'f32+winograd4+x6head'])
def test_full_forward_bs64_vs_oracle(network, cdt):
    """BASELINE configs[1] at ITS OWN size: B = 64 @224, four streams on the liveness-packed
    arena, the tile instantiations the dispatcher picks at this M.  features / betas /
    vertices / joints / measurements against the CPU oracle at 1e-4."""
    x_np, ref = _oracle_bs64()
    x = torch.from_numpy(x_np).cuda()
    network.backbone.multi_stream = True
    network.backbone.compute_dtype = cdt.split('+')[0]
    network.backbone.conv_algo = {'winograd': 'auto', 'winograd4': 'winograd4'}.get(
        (cdt.split('+') + [''])[1], 'direct')
    keep_x6 = network.backbone.x6_gemm_min_batch
    network.backbone.x6_gemm_min_batch = 64 if cdt.endswith('x6head') else keep_x6      # (opt-in: head GEMMs on bf16x6)
    try:
        with torch.no_grad():
            out = network(x, None)
        torch.cuda.synchronize()
    finally:
        network.backbone.compute_dtype = 'f32'
        network.backbone.conv_algo = 'direct'
        network.backbone.x6_gemm_min_batch = keep_x6
    st, rs = out['stage_02'], ref['stages'][-1]
    errs = {
        'features': np.abs(out['features'].cpu().numpy() - ref['features']).max(),
        'betas': np.abs(st['betas'].cpu().numpy() - rs['betas']).max(),
        'vertices': np.abs(st['vertices'].cpu().numpy() - rs['vertices']).max(),
        'v_shaped': np.abs(st['v_shaped'].cpu().numpy() - rs['v_shaped']).max(),
        'joints': np.abs(st['joints']._t.cpu().numpy() - rs['joints']).max(),
    }
    for k in ('mass', 'height', 'chest', 'waist', 'hips'):
        errs['meas_' + k] = np.abs(out['measurements'][k].cpu().numpy() - ref['measurements'][k]).max()
    for k, v in errs.items():
        print(f'bs64 {cdt} {k:14s} {v:.3e}')
    assert int(network.body_measurements.last_overflow.item()) == 0
    bad = {k: v for k, v in errs.items() if not v < 1e-4}
    assert not bad, bad


def test_smplx_dynamic_landmark_lut_clamp_vs_reference_golden(network, golden_dir):
    """Head yaw through and beyond the 39-degree clamp of the contour-landmark LUT
    (lbs.py:35-42; tests/golden/make_golden_lut.py ran the REAL reference SMPLX.forward)."""
    g = np.load(osp.join(golden_dir, 'ops_golden_lut.npz'))
    rot = torch.from_numpy(g['rot']).cuda()
    with torch.no_grad():
        so = network.model(global_rot=rot[:, :1], body_pose=rot[:, 1:],
                           betas=torch.from_numpy(g['betas']).cuda(), get_skin=True,
                           return_shaped=True)
    torch.cuda.synchronize()
    ej = np.abs(so['joints']._t.cpu().numpy() - g['joints']).max(axis=(1, 2))
    ev = np.abs(so['vertices'].cpu().numpy()[:, ::SUB] - g['vertices_sub']).max()
    print('LUT rows', g['lut_rows'], 'joint err per body', ej, 'vertices', ev)
    assert ej.max() < 1e-4 and ev < 1e-4


def test_measurements_1000_meshes_vs_oracle(network):
    """BASELINE configs[3] mesh by mesh: all 1,000 meshes against the C oracle + scipy hull."""
    import bench
    from oracle import measure as om
    faces, v_np = bench.config4_meshes(1000, seed=0)
    lm = om.load_landmarks(osp.join(DATA, 'measurement_defitions.yaml'),
                           osp.join(DATA, 'smplx_measurements.yaml'))
    ref = om.body_measurements(v_np[:, faces], lm)
    bm = network.body_measurements
    out = bm.forward_vertices(torch.from_numpy(v_np).cuda(), torch.from_numpy(faces).cuda())
    out = out.cpu().numpy()
    assert bm.check_overflow() == 0
    for i, k in enumerate(('mass', 'height', 'chest', 'waist', 'hips')):
        err = np.abs(out[:, i] - ref[k])
        print(f'config4 {k:7s} max err {err.max():.3e} (mesh {err.argmax()})')
        np.testing.assert_allclose(out[:, i], ref[k], rtol=5e-6 if k != 'mass' else 2e-5,
                                   atol=2e-6, err_msg=k)
    assert abs(out[0, 2] - 0.8745367) < 2e-6      # mesh 0 is the shipped sample


def _prism(K, radius, y0, y1, jitter=None):
    """Open K-sided prism around the y axis: 2K side triangles (vertices 0..2K-1)."""
    ang = 2 * np.pi * np.arange(K) / K
    r = np.full(K, radius, np.float64) if jitter is None else radius * (1 + jitter)
    bot = np.stack([r * np.cos(ang), np.full(K, y0), r * np.sin(ang)], 1)
    top = np.stack([r * np.cos(ang), np.full(K, y1), r * np.sin(ang)], 1)
    v = np.concatenate([bot, top]).astype(np.float32)
    f = []
    for i in range(K):
        j = (i + 1) % K
        f += [[i, j, K + j], [i, K + j, K + i]]
    return v, np.asarray(f, np.int32)


def _with_landmarks(v, f, heights):
    """Prepends 5 tiny landmark triangles (faces 0..4: head, heel, chest, waist, hips) far away
    from the planes' cross-sections (x = 5: outside the [-1,1] plane quad)."""
    lv, lf = [], []
    for i, h in enumerate(heights):
        lv += [[5.0, h, 5.0], [5.1, h, 5.0], [5.0, h, 5.1]]
        lf.append([3 * i, 3 * i + 1, 3 * i + 2])
    lv = np.asarray(lv, np.float32)
    v2 = np.concatenate([lv, v]).astype(np.float32)
    f2 = np.concatenate([np.asarray(lf, np.int32), f + len(lv)]).astype(np.int32)
    lm = ([0, 1, 2, 3, 4], [[1 / 3, 1 / 3, 1 / 3]] * 5)
    return v2, f2, lm


def _oracle_lm(lm):
    names = ('head_top', 'left_heel', 'chest', 'waist', 'hips')
    return {n: (int(lm[0][i]), np.asarray(lm[1][i], np.float32)) for i, n in enumerate(names)}


def test_hull_edge_cases_vs_oracle(network):
    """Duplicate points, max_collisions overflow (lowest faces kept, as in the ascending-order
    oracle), the reference's `collision_faces > 0` rule (face 0 dropped,
    body_measurements.py:161), and the inputs on which the reference itself raises
    (fewer than 3 points / collinear points: scipy QhullError) -> documented values."""
    from oracle import measure as om
    from scipy.spatial import QhullError
    bm = network.body_measurements
    r = np.random.default_rng(5)
    heights = [0.9, -0.9, 0.31, 0.02, -0.37]          # head, heel, chest, waist, hips

    def run(v, f, lm, mc):
        out = bm.forward_vertices(torch.from_numpy(v[None]).cuda(), torch.from_numpy(f).cuda(),
                                  landmarks=lm, max_collisions=mc).cpu().numpy()[0]
        return out, int(bm.last_overflow.item())

    # (1) jittered 40-gon, every triangle twice (exact duplicate points), no overflow
    v, f = _prism(40, 0.4, -0.8, 0.8, jitter=0.2 * r.uniform(-1, 1, 40))
    v, f, lm = _with_landmarks(v, np.concatenate([f, f]), heights)
    ref = om.body_measurements(v[None][:, f], _oracle_lm(lm), max_collisions=256)
    out, ov = run(v, f, lm, 256)
    assert ov == 0 and om.mesh_to_mesh_forward.last_dropped == 0
    # perimeters of O(3 m) summed over 40 float32 edges in a different order than Qhull's
    # simplices: 4e-6 relative
    for i, k in enumerate(('height', 'chest', 'waist', 'hips'), start=1):
        assert abs(out[i] - ref[k][0]) < 4e-6 * max(1.0, ref[k][0]), (k, out[i], ref[k][0])
    # (2) the same mesh with max_collisions = 16: 160 hits per plane, the 16 lowest faces of each
    # plane triangle survive in the oracle and on the GPU alike; the excess is reported
    ref16 = om.body_measurements(v[None][:, f], _oracle_lm(lm), max_collisions=16)
    dropped = 0
    for h in heights[2:]:
        om.mesh_to_mesh_forward(om.plane_triangles(np.float32([h])), v[None][:, f], 16)
        dropped += om.mesh_to_mesh_forward.last_dropped
    assert dropped > 100
    out16, ov16 = run(v, f, lm, 16)
    assert ov16 == dropped
    for i, k in enumerate(('chest', 'waist', 'hips'), start=2):
        assert abs(out16[i] - ref16[k][0]) < 4e-6 * max(1.0, ref16[k][0]), (k, out16[i], ref16[k][0])
        assert abs(out16[i] - out[i]) > 1e-3            # truncated: a different polygon
    with pytest.warns(UserWarning):
        assert bm.check_overflow() == ov16
    # (3) face 0 is dropped: make face 0 a big triangle through all three planes (the head
    # landmark moves to the end of the table); with it the hull would be much larger
    v3_, f3_ = _prism(24, 0.3, -0.8, 0.8)
    v3_, f3_, lm3 = _with_landmarks(v3_, f3_, heights)
    big = np.asarray([[-0.9, -0.85, -0.9], [0.9, 0.0, 0.9], [-0.9, 0.85, 0.9]], np.float32)
    nv = len(v3_)
    v3b = np.concatenate([v3_, big]).astype(np.float32)
    f3b = np.concatenate([[[nv, nv + 1, nv + 2]], f3_[1:], f3_[:1]]).astype(np.int32)
    lm3b = ([len(f3b) - 1, 1, 2, 3, 4], lm3[1])
    ref3 = om.body_measurements(v3b[None][:, f3b], _oracle_lm(lm3b))
    out3, _ = run(v3b, f3b, lm3b, 256)
    base3, _ = run(v3_, f3_, lm3, 256)
    for i, k in enumerate(('chest', 'waist', 'hips'), start=2):
        assert abs(out3[i] - ref3[k][0]) < 4e-6 * max(1.0, ref3[k][0]), k
        assert abs(out3[i] - base3[i]) < 4e-6 * max(1.0, base3[i]), k   # as if the big triangle were not there
    # (4) the reference raises on degenerate cross-sections; the kernel returns 0 for fewer
    # than 2 points and twice the segment length for collinear points
    flat_v = np.asarray([[-0.5, -0.8, 0.0], [0.5, -0.8, 0.0], [0.5, 0.8, 0.0], [-0.5, 0.8, 0.0]],
                        np.float32)
    flat_f = np.asarray([[0, 1, 2], [0, 2, 3]], np.int32)
    v4, f4, lm4 = _with_landmarks(flat_v, flat_f, heights)
    with pytest.raises(QhullError):
        om.body_measurements(v4[None][:, f4], _oracle_lm(lm4))
    out4, _ = run(v4, f4, lm4, 256)
    for i in (2, 3, 4):
        assert 0.0 < out4[i] <= 2.0 + 1e-5 and np.isfinite(out4[i])
    v5, f5, lm5 = _with_landmarks(flat_v[:3] + np.float32([0, 5, 0]), flat_f[:1], heights)
    out5, _ = run(v5, f5, lm5, 256)                    # nothing crosses any plane
    assert out5[2] == 0 and out5[3] == 0 and out5[4] == 0
    assert abs(out5[1] - 1.8) < 1e-6


def _nccl_worker(rank, world, port, q, backend='nccl'):
    """backend 'nccl': one GPU per rank, the betas gathered by RCCL; 'gloo': the ranks share GPU 0
    (RCCL refuses two ranks on one device) and gather the betas over gloo from host memory."""
    import os
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), LOCAL_RANK=str(rank), HSA_ENABLE_IPC_MODE_LEGACY='0')
    import torch.distributed as dist
    import __graft_entry__ as ge
    from shapy_amd import parallel
    from shapy_amd.utils import synthetic as syn
    torch.cuda.set_device(rank if backend == 'nccl' else 0)
    dist.init_process_group(backend, init_method='env://')
    try:
        net, _ = ge.make_network()
        xs = [torch.from_numpy(syn.synthetic_images(2, 64, 100 + r)).cuda() for r in range(world)]
        gat = parallel.BetasGatherer(world)
        to = (lambda t: t) if backend == 'nccl' else (lambda t: t.cpu())
        with torch.no_grad():
            mine = net(xs[rank], None)['stage_02']['betas']
            g1 = gat(to(mine))
            g2 = gat(to(mine + 1))              # second step: joins the first gather
            gat.wait()
            others = to(torch.cat([net(x, None)['stage_02']['betas'] for x in xs]))
        torch.cuda.synchronize()
        ok = (torch.equal(g1, others) and torch.equal(g2, others + 1) and gat.deferred_waits == 1)
        q.put((rank, bool(ok)))
    finally:
        dist.destroy_process_group()


def _nccl_one_rank_worker(port, q):
    import os
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK='0', WORLD_SIZE='1',
                      LOCAL_RANK='0', HSA_ENABLE_IPC_MODE_LEGACY='0')
    import torch.distributed as dist
    from shapy_amd import parallel
    torch.cuda.set_device(0)
    dist.init_process_group('nccl', init_method='env://')
    try:
        ok = {}
        for mode in ('lane', 'work'):
            gat = parallel.BetasGatherer(1, force=True, mode=mode)
            side = torch.cuda.Stream()
            with torch.cuda.stream(side):              # a non-default caller stream, as in serving
                xs = [torch.randn(64, 10, device='cuda') for _ in range(3)]
                outs = [gat(x * 2) for x in xs]        # three "steps": two deferred joins
                last = gat.wait()
            torch.cuda.synchronize()
            ok[mode] = (all(torch.equal(o, x * 2) for o, x in zip(outs, xs)) and last is outs[-1]
                        and gat.issued == 3 and gat.deferred_waits == 2 and gat.wait() is None)
            gat.close()
        # the direct communicator "fails" on every rank -> the gatherer agrees on c10d (mode 'work')
        os.environ['SHAPY_RCCL_FORCE_FAIL'] = '1'
        gat = parallel.BetasGatherer(1, force=True, mode='lane')
        x = torch.randn(8, 10, device='cuda')
        got = gat.gather(x)
        torch.cuda.synchronize()
        ok['fallback'] = bool(torch.equal(got, x) and gat.mode == 'work')
        del os.environ['SHAPY_RCCL_FORCE_FAIL']
        q.put(ok)
    finally:
        dist.destroy_process_group()


def test_rccl_forced_gather_one_rank_both_modes():
    """bench.py --force-gather's path: a world-size-1 RCCL group on ONE GPU runs the collective of the
    N-rank path in both issue modes of BetasGatherer ('lane', the default: ncclAllGather called
    directly on the executor's lane-1 stream and joined one step later, shapy_amd/rccl.py; 'work': the
    fallback, c10d async collective from the caller's stream) and the agreed fallback itself."""
    _need_gpu()
    import socket
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    p = ctx.Process(target=_nccl_one_rank_worker, args=(port, q))
    p.start()
    res = q.get(timeout=300)
    p.join(timeout=60)
    assert res == {'lane': True, 'work': True, 'fallback': True}, res


def test_rccl_allgather_two_ranks():
    """The N > 1 path: two ranks, each running the HIP network on its own shard; every rank's gathered
    betas equal what it computes itself for all shards (same weights, deterministic kernels), the
    second step joining the first gather.  With two GPUs: one GPU per rank, gathered by real RCCL.
    With one GPU the two ranks share it and gather over gloo -- RCCL refuses two ranks on one device;
    its collective on one rank is test_rccl_forced_gather_one_rank_both_modes."""
    _need_gpu()
    backend = 'nccl' if torch.cuda.device_count() >= 2 else 'gloo'
    import socket
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_nccl_worker, args=(r, 2, port, q, backend)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=600) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    assert res == [(0, True), (1, True)]
