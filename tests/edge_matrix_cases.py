"""The kernels around the UNet of the volume path -- k_conv_f32 (the fp32-operand conv), k_vq_lookup, k_stem1 / k_stem2, k_conv_c1 and
k_layernorm: the cases, their inputs and their float64 references.  Shared by tests/test_edge_matrix_cpu.py (the conditions the cases
themselves have to meet, no GPU), tests/test_hip_conv32_matrix.py and tests/test_hip_edge_matrix.py (the launches, against float64).
A plain module: no fixtures, no test.

MARGIN = 16 is the conv matrix's: a kernel performs the same number of fp32 roundings as the fp32 CPU computation in another order, for
which a factor of a few is expected; a wrong tap, window, mask or statistic is off by 1e-2 and more."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import conv_matrix_cases as cm

MARGIN = 16
U = 2.0 ** -24            # unit roundoff of fp32


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _rnd(shape, seed, scale=1.0):
    return torch.randn(shape, generator=_gen(seed), dtype=torch.float32) * scale


# ---- 1. k_conv_f32 ---------------------------------------------------------------------------------------------------------------------
# the conv matrix's families (A: 5 objects of 4x4x8 = five 128-row tiles of one object each, per-object vector; B: 5 objects of 2x4x4 =
# 160 rows, the second 128-row tile ragged, tiles straddling objects; 64 -> 232 columns = 64 + 64 + 64 + 40), all six modes, the
# 96-channel fused skip in the four modes that take one; bias and residual everywhere.  One fp32 output, one kernel: no routes.
def _of_family(c):
    d = {k: v for k, v in c.items() if k not in ('routes', 'stats')}
    d.update(name='f32-' + c['name'], out='f32')
    return d


def _same32(name, O, dims, taps, Cin, N, rowvec=False, res=False, out='f32'):
    return dict(name=name, family=None, O=O, dims=dims, taps=taps, Cin=Cin, N=N, mode=cm.SAME, Cin2=0, rowvec=rowvec, res=res, out=out,
                geglu=False)


CONV32_CASES = [_of_family(c) for c in cm.FAMILY_CASES] + [
    _same32('f32-linear', 5, (2, 4, 4), 1, 64, 232, res=True),                       # taps = 1
    _same32('f32-cin40', 3, (2, 4, 4), 27, 40, 72, rowvec=True, res=True),           # 40 -> 48 channels: es_pack_conv_f32's zero fill
    _same32('f32-ncdhw-n3', 2, (4, 4, 4), 27, 64, 3, out='ncdhw'),                   # the output conv's form
    _same32('f32-m8', 1, (2, 2, 2), 27, 32, 72, rowvec=True, res=True),              # one tile, 8 of its 128 rows live
]


# ---- 2. k_vq_lookup --------------------------------------------------------------------------------------------------------------------
VQ_CASES = [
    dict(name='n64-m200', n_embed=64, O=2, V=100, Cpad=32),           # less than one workgroup, the object boundary inside it
    dict(name='n320-m4200', n_embed=320, O=3, V=1400, Cpad=8),        # codebook not a multiple of 256, 17 workgroups, ragged last
    dict(name='n8192-m1040', n_embed=8192, O=2, V=520, Cpad=32),      # the product's codebook and dynamic LDS size
    dict(name='n320-cpad3', n_embed=320, O=2, V=300, Cpad=3),         # no padding
]
VQ_FAMILIES = ('varied', 'on_code', 'duplicates', 'near_ties')
VQ_TIE_FACTOR = 64        # a decidable near-tie: the float64 gap of the two distances is 64 x the bound
VQ_NDUP = 8


def vq_dist(z, e):
    """float64 [M, n]: |z|^2 + |e|^2 - 2 z.e, and S = |z|^2 + |e|^2 + 2 sum_i |z_i e_i|, the magnitude the fp32 roundings act on"""
    z, e = z.astype(np.float64), e.astype(np.float64)
    zz, ee = (z * z).sum(1)[:, None], (e * e).sum(1)[None, :]
    return zz + ee - 2.0 * (z @ e.T), zz + ee + 2.0 * (np.abs(z) @ np.abs(e).T)


def vq_bound(S):
    """16 u S: the kernel's expression is three roundings in each squared norm, one in their sum, at most three in the dot product and
    one in the subtraction -- under 8 u S per candidate, and two candidates take part"""
    return 16 * U * S


def _two_smallest(D):
    i0 = D.argmin(1)
    r = np.arange(D.shape[0])
    d0 = D[r, i0]
    D2 = D.copy()
    D2[r, i0] = np.inf
    i1 = D2.argmin(1)
    return i0, d0, i1, D2[r, i1], D2


@functools.lru_cache(maxsize=None)
def _vq_tables(name):
    case = next(c for c in VQ_CASES if c['name'] == name)
    n, M = case['n_embed'], case['O'] * case['V']
    rng = np.random.default_rng(1000 + n + M)
    codebook = rng.standard_normal((n, 3)).astype(np.float32)
    lut = rng.standard_normal((n, 3)).astype(np.float32)
    # candidate codes for the families that sit on or between codes: a code and its nearest other code, kept where that neighbour
    # is decidably farther (the gap of the float64 distances from the code itself exceeds VQ_TIE_FACTOR x the bound)
    cand = rng.permutation(n)[:min(n, max(M, 256))]
    D, S = vq_dist(codebook[cand], codebook)
    r = np.arange(len(cand))
    D[r, cand] = np.inf                                   # (the code itself)
    nb = D.argmin(1)
    ok = D[r, nb] > VQ_TIE_FACTOR * vq_bound(np.maximum(S[r, nb], S[r, cand]))
    return codebook, lut, cand[ok], nb[ok]


@functools.lru_cache(maxsize=2)
def vq_problem(name, family):
    """z f32 [O, 3, V], codebook and lut f32 [n, 3], `want` (the index every voxel must get; None: any index within the bound),
    D and S float64 [M, n] of exactly these operands"""
    case = next(c for c in VQ_CASES if c['name'] == name)
    n, O, V = case['n_embed'], case['O'], case['V']
    M = O * V
    codebook, lut, codes, nbs = _vq_tables(name)
    codebook, lut = codebook.copy(), lut.copy()
    rng = np.random.default_rng(7 + n + M + VQ_FAMILIES.index(family))
    want = None
    if family == 'varied':
        z = (0.8 * rng.standard_normal((M, 3))).astype(np.float32)
    elif family == 'on_code':
        want = np.resize(codes, M)
        z = codebook[want]
    elif family == 'duplicates':
        # rows j1 < j2 equal (codebook and lut): the first minimum is j1.  j1: decidable codes from the front; j2: the row behind the
        # first j1, and rows from the end of the codebook
        j1 = np.sort(codes[codes < n - VQ_NDUP - 1])[:VQ_NDUP]
        j2 = np.array([j1[0] + 1 if j1[0] + 1 not in j1 else n - VQ_NDUP] + [n - 1 - i for i in range(VQ_NDUP - 1)])
        assert len(j1) == VQ_NDUP and bool((j1 < j2).all()) and not set(j1) & set(j2)
        codebook[j2], lut[j2] = codebook[j1], lut[j1]
        want = np.resize(j1, M)
        z = codebook[want]
    else:
        # z = (e_a + e_b) / 2 + delta (e_b - e_a), b the nearest code of a: D(a) - D(b) = 2 delta |e_b - e_a|^2, delta = +- the value that
        # makes it VQ_TIE_FACTOR x the bound (pairs that need |delta| > 1/4 are left out); + lands on b, - on a
        ea, eb = codebook[codes].astype(np.float64), codebook[nbs].astype(np.float64)
        mid, dl = 0.5 * (ea + eb), eb - ea
        Smid = np.maximum(vq_dist(mid, codebook[codes])[1].diagonal(), vq_dist(mid, codebook[nbs])[1].diagonal())
        delta = 0.5 * VQ_TIE_FACTOR * vq_bound(Smid) / (dl * dl).sum(1)
        use = np.nonzero(delta <= 0.25)[0]
        for s in (1.0, -1.0):
            # ... and pairs where a third code is not decidably farther than the pair, on either side
            Dt, St = vq_dist((mid[use] + s * delta[use, None] * dl[use]).astype(np.float32), codebook)
            r = np.arange(len(use))
            dpair, spair = np.minimum(Dt[r, codes[use]], Dt[r, nbs[use]]), np.maximum(St[r, codes[use]], St[r, nbs[use]])
            Dt[r, codes[use]] = Dt[r, nbs[use]] = np.inf
            t = Dt.argmin(1)
            use = use[Dt[r, t] - dpair > VQ_TIE_FACTOR * vq_bound(np.maximum(St[r, t], spair))]
        assert len(use) >= 8, 'too few decidable pairs'
        k = np.resize(use, M)
        sign = np.where(np.arange(M) // len(use) % 2 == 0, 1.0, -1.0) * np.where(np.arange(M) % 2 == 0, 1.0, -1.0)
        z = (mid[k] + (sign * delta[k])[:, None] * dl[k]).astype(np.float32)
        want = np.where(sign > 0, nbs[k], codes[k])
        pair = np.stack([codes[k], nbs[k]], 1)
    D, S = vq_dist(z, codebook)
    p = dict(case=case, family=family, z=np.ascontiguousarray(z.reshape(O, V, 3).transpose(0, 2, 1)), codebook=codebook, lut=lut,
             want=want, D=D, S=S)
    if family == 'near_ties':
        p['pair'] = pair
    return p


def vq_undecided_share(p):
    """the share of voxels whose float64 best and second best lie within the bound of each other"""
    i0, d0, i1, d1, _ = _two_smallest(p['D'])
    r = np.arange(len(i0))
    return float((d1 - d0 <= vq_bound(np.maximum(p['S'][r, i0], p['S'][r, i1]))).mean())


def vq_check_indices(p, idx):
    """findings of the indices a launch returned: out of range, beyond the bound, not the index the family pins; and the number of
    voxels that differ from the float64 first minimum"""
    D, S, n = p['D'], p['S'], p['case']['n_embed']
    bad = []
    idx = np.asarray(idx).astype(np.int64)
    if ((idx < 0) | (idx >= n)).any():
        return ['%d indices outside 0..%d (never written?)' % (int(((idx < 0) | (idx >= n)).sum()), n - 1)], -1
    r = np.arange(len(idx))
    best = D.argmin(1)                                     # (numpy: the first minimum)
    over = D[r, idx] - D[r, best] - vq_bound(np.maximum(S[r, idx], S[r, best]))
    if (over > 0).any():
        m = int(over.argmax())
        bad.append('%d voxels got a code whose float64 distance is beyond the bound above the minimum; worst voxel %d: code %d at %.9g, '
                   'best %d at %.9g, bound %.3g' % (int((over > 0).sum()), m, idx[m], D[m, idx[m]], best[m], D[m, best[m]],
                                                    vq_bound(max(S[m, idx[m]], S[m, best[m]]))))
    if p['want'] is not None and (idx != p['want']).any():
        m = int(np.nonzero(idx != p['want'])[0][0])
        bad.append('%d voxels did not get the code the family pins; first: voxel %d got %d, must get %d'
                   % (int((idx != p['want']).sum()), m, idx[m], p['want'][m]))
    return bad, int((idx != best).sum())


# ---- 3. the conv-pool stem -------------------------------------------------------------------------------------------------------------
STEM_LAUNCHES = [(O, cin, gap) for O in (1, 3) for cin in (3, 4) for gap in (0, 52)]      # x_ostride = 0, or cin * 4096 + gap
STEM_FAMILIES = ('varied', 'all_negative', 'far_window')


@functools.lru_cache(maxsize=None)
def stem_problem(O, cin, family):
    """x f32 [O, cin, 16, 16, 16], (w0 [32, cin, 3, 3, 3], b0, w1 [64, 32, 3, 3, 3], b1)"""
    x = _rnd((O, cin, 16, 16, 16), 21)
    w0, b0 = _rnd((32, cin, 3, 3, 3), 22) / np.sqrt(27 * cin), _rnd((32,), 23)
    w1, b1 = _rnd((64, 32, 3, 3, 3), 24) / np.sqrt(27 * 32), _rnd((64,), 25)
    if family == 'all_negative':
        # every conv output and every pooled value below zero: a pool that starts at 0 instead of -inf, or a halo that is not zero, shows
        w0, b0 = 0.3 * w0, -4.0 + 0.1 * b0
        w1, b1 = 0.05 * w1, -4.0 + 0.1 * b1
    if family == 'far_window':
        # non-zero only in the octants of conv outputs that the stride-4 pool of stage 2 does not read -- indices 2, 3, 6, 7 of each
        # axis of the 8^3 map (voxels 4..7 and 12..15 of the 16^3 input; the convs spread them by one voxel of halo), and large there
        keep = torch.zeros(16, dtype=torch.bool)
        keep[4:8] = keep[12:16] = True
        x = 8.0 * x * (keep[:, None, None] & keep[None, :, None] & keep[None, None, :])
    return x.contiguous(), (w0.contiguous(), b0.contiguous(), w1.contiguous(), b1.contiguous())


def stem_reference(x, w, dt, start=4):
    """the four layers of the stem (Conv3d(k3, p1), MaxPool3d(2, 2), Conv3d(k3, p1), MaxPool3d(k = 2, s = 4)) and the flatten, in
    ``dt``: the stage-1 map [O, 32, 8, 8, 8], the conv of stage 2 [O, 64, 8, 8, 8] and the output [O, 512].  ``start``: where the
    second pooling window of an axis begins (4; the CPU file moves it to show what the far-window family is for)"""
    w0, b0, w1, b1 = (t.to(dt) for t in w)
    h1 = F.max_pool3d(F.conv3d(x.to(dt), w0, b0, padding=1), kernel_size=2, stride=2)
    c2 = F.conv3d(h1, w1, b1, padding=1)
    ix = torch.tensor([0, 1, start, start + 1])
    win = c2[:, :, ix][:, :, :, ix][:, :, :, :, ix]                         # the voxels the two windows of each axis cover
    out = F.max_pool3d(win, kernel_size=2, stride=2)
    return h1, c2, out.flatten(1)


# ---- 4. k_conv_c1 ----------------------------------------------------------------------------------------------------------------------
C1_CASES = [(N, dims) for N in (16, 32, 64, 128) for dims in ((4, 4, 16), (8, 8, 32))]      # O = 2 everywhere
C1_O = 2
C1_OUTPUTS = ('f32', 'f16', 'both')


@functools.lru_cache(maxsize=None)
def c1_problem(N, dims):
    x = _rnd((C1_O, 1) + dims, 31)
    wt = _rnd((N, 1, 3, 3, 3), 32) / np.sqrt(27)
    bias = _rnd((N,), 33)
    out = {}
    for with_bias in (True, False):
        ref = F.conv3d(x.double(), wt.double(), bias.double() if with_bias else None, padding=1)
        y32 = F.conv3d(x, wt, bias if with_bias else None, padding=1)
        scale = ref.abs().max().item()
        out[with_bias] = dict(ref=ref.permute(0, 2, 3, 4, 1).reshape(-1, N).contiguous(), scale=scale,
                              e32=(y32.double() - ref).abs().max().item() / scale)
    return x, wt, bias, out


# ---- 5. k_layernorm --------------------------------------------------------------------------------------------------------------------
LN_SHAPES = [(3, 8), (37, 1024), (5, 100), (6, 260), (8197, 448)]
LN_FAMILIES = ('varied', 'ratio10', 'ratio1000', 'const_row')
LN_EPS = 1e-5
LN_CONST = (0.7, -3.0, 1000.0)          # the constant rows: first, middle and last row


@functools.lru_cache(maxsize=None)
def ln_problem(M, C, family):
    """x f32 [M, C], gamma, beta f32 [C] (order 1, both signs)"""
    x = _rnd((M, C), 41)
    sign = lambda t: torch.where(t < 0.5, -1.0, 1.0)
    if family.startswith('ratio'):
        spread = 0.5 + 1.5 * torch.rand(M, 1, generator=_gen(42))
        mean = float(family[5:]) * spread * sign(torch.rand(M, 1, generator=_gen(43)))
    else:
        spread = 0.25 + 2.0 * torch.rand(M, 1, generator=_gen(42))
        mean = 2.0 * _rnd((M, 1), 43)
    x = x * spread + mean
    if family == 'const_row':
        for row, c in zip((0, M // 2, M - 1), LN_CONST):
            x[row] = c
    gamma = (0.5 + torch.rand(C, generator=_gen(44))) * sign(torch.rand(C, generator=_gen(45)))
    beta = (0.05 + torch.rand(C, generator=_gen(46))) * sign(torch.rand(C, generator=_gen(47)))
    return x.contiguous(), gamma, beta


def ln_reference(x, gamma, beta):
    """float64 LayerNorm (biased variance, the kernel's fp32 eps), and the magnitude w the fp32 roundings act on, per element:
    |gamma| (|x - mean| + |mean|) rstd + |beta| -- the row's conditioning 1 + |mean| rstd sits on the normalised term: an error of
    k u |mean| in the mean moves every element of the row by that times rstd |gamma|.  (No 1 + r^2 term: the statistics are a centred
    sum; E[x^2] - mean^2 would need one.)"""
    xd, ga, be = x.double(), gamma.double(), beta.double()
    mean = xd.mean(1, keepdim=True)
    d = xd - mean
    rstd = 1.0 / torch.sqrt((d * d).mean(1, keepdim=True) + float(torch.tensor(LN_EPS, dtype=torch.float32)))
    return d * rstd * ga + be, ga.abs() * (d.abs() + mean.abs()) * rstd + be.abs()


def ln_two_pass_fp32(x, gamma, beta):
    """the yardstick: the same two-pass LayerNorm in fp32 on the CPU"""
    C = x.shape[1]
    mean = x.sum(1, keepdim=True) / C
    d = x - mean
    rstd = 1.0 / torch.sqrt((d * d).sum(1, keepdim=True) / C + torch.tensor(LN_EPS, dtype=torch.float32))
    return d * rstd * gamma + beta


def ln_yardstick(x, gamma, beta):
    """ref, w and E = the largest |fp32 CPU - float64| / w"""
    ref, w = ln_reference(x, gamma, beta)
    return ref, w, ((ln_two_pass_fp32(x, gamma, beta).double() - ref).abs() / w).max().item()


def all_case_names():
    return ([c['name'] for c in CONV32_CASES] + ['vq-%s-%s' % (c['name'], f) for c in VQ_CASES for f in VQ_FAMILIES] +
            ['stem-o%d-c%d-g%d-%s' % (l + (f,)) for l in STEM_LAUNCHES for f in STEM_FAMILIES] +
            ['c1-n%d-%dx%dx%d' % ((N,) + d) for N, d in C1_CASES] + ['ln-%dx%d-%s' % (M, C, f) for M, C in LN_SHAPES for f in LN_FAMILIES])
