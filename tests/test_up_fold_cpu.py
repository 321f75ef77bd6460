"""CPU-only: the folded weights of the up-sampling convs (nearest x2 on H and W, then 3x3x3: per output parity a 3x2x2 conv on the input
grid, 12 taps instead of 27), the packed image the kernel streams, and the route that multiplies through it.

  * plan_vol.up_fold_weights applied as four 3x2x2 convs reproduces F.conv3d(F.interpolate(x, nearest x(1, 2, 2)), w, padding=1) in
    float64, borders included (Hi = Wi = 2: every voxel touches a face);
  * es_pack_conv_up_fold_f16 holds exactly those sums, rounded to f16 once, in the tiled and swizzled layout of es_pack_conv_f16 (four
    class images of a 12-tap conv), zero in the padding of a ragged column tile and of a channel count that is no multiple of 32;
  * es_conv_kernel_of names the folded route for an eligible launch and today's kernel for each reason a launch is not eligible.
No device compute."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_conv_route_cpu import _options, _set

UP_HW = 2
FOLD = 'ws_256_up_fold'


@pytest.fixture(scope='module')
def L():
    import __graft_entry__ as ge
    ge.build()
    from echoscene_amd import hip
    return hip.lib()


def _rnd(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


def folded_conv(x, Wf):
    """the four 3x2x2 convs of the folded weights Wf [4, N, Cin, 3, 2, 2] on x [O, Cin, D, Hi, Wi], interleaved into [O, N, D, 2 Hi, 2 Wi]"""
    O, _, D, Hi, Wi = x.shape
    y = torch.zeros(O, Wf.shape[1], D, 2 * Hi, 2 * Wi, dtype=x.dtype)
    for ph in (0, 1):
        for pw in (0, 1):
            # parity 0 reads input rows hi - 1, hi (zero in front of the first), parity 1 reads hi, hi + 1 (zero behind the last)
            xp = F.pad(x, (1 - pw, pw, 1 - ph, ph, 1, 1))
            y[:, :, :, ph::2, pw::2] = F.conv3d(xp, Wf[2 * ph + pw])
    return y


@pytest.mark.parametrize('dims', [(2, 2, 2), (3, 3, 4), (1, 1, 1)], ids=lambda d: 'x'.join(map(str, d)))
def test_folded_weights_reproduce_the_up_sampling_conv(dims):
    from echoscene_amd.plan_vol import up_fold_weights
    D, Hi, Wi = dims
    x, w = _rnd((2, 5, D, Hi, Wi), 1).double(), _rnd((7, 5, 3, 3, 3), 2)
    ref = F.conv3d(F.interpolate(x, scale_factor=(1, 2, 2), mode='nearest'), w.double(), padding=1)
    Wf = up_fold_weights(w)
    assert Wf.dtype == torch.float64 and tuple(Wf.shape) == (4, 7, 5, 3, 2, 2)
    got = folded_conv(x, Wf)
    # the same products, summed in another order: a few float64 roundings of K = 135 terms
    assert (got - ref).abs().max().item() <= 1e-13 * ref.abs().max().item()
    # every one of the 27 taps is counted exactly once per class
    assert torch.allclose(Wf.sum((3, 4, 5)), w.double().sum((2, 3, 4)).expand(4, -1, -1), rtol=0, atol=1e-12)


def _unpack(img, N, Cin, taps):
    """[N, Cin, taps] f16 values of a tiled, swizzled image [n-tile of 224][chunk][tap][256 rows x 4 chunks of 8] (es_pack_conv_f16) and
    the sum of |.| over the padding"""
    nt, kch = (N + 223) // 224, Cin // 32
    a = img.view(nt, kch, taps, 256, 4, 8)
    row = torch.arange(256)
    swz = (0x1320 >> (((row >> 2) & 3) * 4)) & 3
    out = torch.empty(nt, kch, taps, 256, 4, 8, dtype=img.dtype)
    for lc in range(4):
        out[:, :, :, row, lc] = a[:, :, :, row, lc ^ swz]                     # physical chunk = logical chunk ^ swizzle(row)
    full = out.permute(0, 3, 1, 4, 5, 2).reshape(nt, 256, Cin, taps)            # [tile, row, channel, tap]
    vals = full[:, :224].reshape(nt * 224, Cin, taps)
    pad = full[:, 224:].float().abs().sum().item() + vals[N:].float().abs().sum().item()
    return vals[:N], pad


@pytest.mark.parametrize('N,cin', [(232, 40), (8, 64)])
def test_packed_image_holds_the_folded_sums_rounded_once(L, N, cin):
    from echoscene_amd.plan_vol import up_fold_weights
    w = _rnd((N, cin, 3, 3, 3), 3) / np.sqrt(cin * 27.0)
    Cin = (cin + 31) // 32 * 32
    n = L.es_pack_conv_up_fold_f16_size(N, Cin)
    assert n == 4 * L.es_pack_conv_f16_size(N, Cin, 12)
    img = torch.full((n,), 0x7e00, dtype=torch.int16)                           # (NaN: every element must be written)
    assert L.es_pack_conv_up_fold_f16(C.c_void_p(w.contiguous().data_ptr()), N, cin, C.c_void_p(img.data_ptr())) == 0
    Wf = up_fold_weights(w)                                                     # [4, N, cin, 3, 2, 2] float64
    want = torch.from_numpy(Wf.numpy().astype(np.float16)).reshape(4, N, cin, 12)       # numpy rounds float64 -> float16 once
    per = n // 4
    for cls in range(4):
        vals, pad = _unpack(img[cls * per:(cls + 1) * per].view(torch.float16), N, Cin, 12)
        assert pad == 0.0
        assert torch.equal(vals[:, :cin].view(torch.int16), want[cls].view(torch.int16)), 'class %d' % cls
        assert vals[:, cin:].float().abs().sum().item() == 0.0


def _args(O, dims, Cin, N, w2=0x2100, workspace=False, splitk=0, o_hint=0, mode=UP_HW):
    from echoscene_amd import hip
    a = hip.ConvArgs()
    a.a, a.w = 0x1000, 0x2000
    a.O, (a.D, a.H, a.W) = O, dims
    a.Cin, a.N, a.taps, a.mode = Cin, N, 27, mode
    a.w2 = w2 or None
    a.bias, a.out_f32, a.out_ld = 0x5000, 0x3000, N
    a.O_hint = o_hint
    if workspace:
        a.workspace, a.splitk = 0x6000, splitk
    return a


def _kernel_of(L, a):
    name = C.create_string_buffer(32)
    S = L.es_conv_kernel_of(C.byref(a), name, 32)
    return name.value.decode(), S


def test_the_folded_route_is_named_for_eligible_launches_only(L):
    found = _options(L)
    try:
        # the two up-sampling launches of the full-width step at 32 objects: the first has no split-K workspace (its output is over
        # the planner's bound), the second has one and is split over K today -- it keeps its route
        big = dict(O=32, dims=(16, 16, 16), Cin=448, N=448)
        assert _kernel_of(L, _args(**big)) == (FOLD, 1)
        assert _kernel_of(L, _args(w2=0, **big)) == ('ws_256_8_4_3', 1)                       # no folded image
        for hint in (-4, 64):                                                                  # canonical / sharded arithmetic
            assert _kernel_of(L, _args(o_hint=hint, **big)) == _kernel_of(L, _args(o_hint=hint, w2=0, **big))
            assert _kernel_of(L, _args(o_hint=hint, **big))[0] != FOLD
        second = dict(O=32, dims=(16, 8, 8), Cin=672, N=672)
        assert _kernel_of(L, _args(**second)) == (FOLD, 1)                                    # unsplit: eligible
        for sk in (-1, 2, 3):                                                                  # a split launch
            got = _kernel_of(L, _args(workspace=True, splitk=sk, **second))
            assert got == _kernel_of(L, _args(workspace=True, splitk=sk, w2=0, **second)) and got[0] != FOLD and got[1] > 1, got
        # D Hi Wi % 256 != 0: a 256-row tile would hold more than one parity class
        odd = dict(O=512, dims=(2, 8, 8), Cin=64, N=448)
        assert _kernel_of(L, _args(**odd)) == _kernel_of(L, _args(w2=0, **odd)) == ('ws_256_8_4_3', 1)
        # not the 256-row producer/consumer kernel: few rows, the non-specialised kernel, the other up-sampling mode
        few = dict(O=2, dims=(16, 8, 8), Cin=64, N=232)
        assert _kernel_of(L, _args(**few)) == _kernel_of(L, _args(w2=0, **few)) and _kernel_of(L, _args(**few))[0] != FOLD
        _set(L, [('conv_force256', 1)])
        assert _kernel_of(L, _args(**few)) == (FOLD, 1)                                       # (what tests/test_hip_up_fold.py launches)
        assert _kernel_of(L, _args(workspace=True, splitk=-1, **few)) == (FOLD, 1)
        assert _kernel_of(L, _args(O=1, dims=(4, 16, 16), Cin=32, N=224)) == (FOLD, 1)
        assert _kernel_of(L, _args(mode=3, **few)) == ('ws_256_8_4_3', 1)                     # UP_DHW
        _set(L, [('conv_ws', 0)])
        assert _kernel_of(L, _args(**few)) == ('lean_256', 1)
    finally:
        _set(L, found)


def test_the_planner_attaches_the_image_where_the_issue_allows_it():
    """host-side only: PackedConv(up_fold=True) forms the image; the step emitter sets w2 on the 'up' conv of a plain fp16 plan and on no other"""
    from echoscene_amd.plan_vol import PackedConv
    w, b = _rnd((8, 32, 3, 3, 3), 5), _rnd((8,), 6)
    pc = PackedConv(w, b, 'cpu', up_fold=True)
    assert pc.w_fold is not None and pc.w_fold.numel() == 4 * 12 * 256 * 32 and pc.taps == 27
    assert PackedConv(w, b, 'cpu').w_fold is None
    assert PackedConv(w.flatten(1)[:, :64].contiguous(), b, 'cpu', up_fold=True).w_fold is None          # a 1x1 weight has nothing to fold
