"""GPU: every instantiation of the two rows kernels (k_rows_x, k_linear_rows) against fp64, with the route asserted.  The cases and
their routes: tests/rows_matrix_cases.py (checked without a GPU by tests/test_rows_matrix_cpu.py).  Launches go through the C ABI
(es_linear_rows_f32 / es_linear_rows_multi_f32) with explicit slices; the prefetch cases run as a two-op plan.

One test per case.  For every launch call:
  * the route: es_linear_rows_route_of on the REAL argument structs names the launches the table names (kernel, fall-back reason, grid,
    block, LDS, prefetch descriptor, per problem S / kbps / Jw / cuts / k-blocks per wave / wg0 / ny / xw / fw), or nothing is launched
    and the test fails;
  * stray accesses (tests/guarded_buffers.py): every operand -- A segments with all their slabs, gather tables and indices, CSR
    sources and entry lists, gamma / beta, bias, residual slabs, the packed weights, the step counter -- sits between NaN guards (the
    columns between a matrix's width and its leading dimension hold NaN too); every output -- each slab, each batch, the published
    LN_ATTN row -- is NaN-filled between patterned guard rows, with out_ld > N and two spare rows between slabs.  No guard changes, no
    element of rows < M, columns < N stays unwritten, nothing else is written, no NaN reaches a result;
  * the values: float64 of the plain formula on the operands as the kernel receives them -- slab sum, input ReLU, prologue (GroupNorm
    per group with biased variance, LayerNorm per row, SiLU, value * gelu(gate), the formed row x = rstd(t0) u + t0 + cav then
    LayerNorm; CSR pooling: entries ReLU'd one by one, weighted ones as sum w v / (sum w + 1e-4)), product, bias, activation, residual
    slab sums (the GEGLU epilogue value * gelu(gate) is the activation: residuals come after it, as the header documents).  Every
    output slab is compared on its own: slab 0 carries bias and residuals, slab s the bare partial product of slice s.
    The bound is PER ELEMENT:  err <= s * scale (+ derived terms),  scale = sum_k |a_k| |w_k| + |bias| + sum |residual slabs| with a the
    fp64 prologue output, carried through an activation by the bound of its derivative (ReLU 1, SiLU 1.1, sigmoid 0.25, GEGLU:
    |gelu(g)| dv + 1.13 |v| dg).  s is one number per class, 4 x the largest value measured on an MI355X rounded up to one digit
    (every run prints each case's figure under -s):
        plain operands           measured 2.14e-7 (f0-7-slices)              bar 9e-7  (ceiling 1e-5: under 90 roundings, 90 x 2^-24 = 5.4e-6)
        GroupNorm prologue       measured 6.30e-7 (F0-u1-gn-2slab)           bar 3e-6  (ceiling 1e-4)
        LayerNorm / formed row   measured 2.25e-7 (xlnattn-const-t0-row, the published row)  bar 9e-7  (ceiling 1e-4)
        expf epilogue / SiLU, GEGLU prologue   measured 1.71e-7 (xlnattn-nt2-w128, the published row)   bar 7e-7  (ceiling 1e-4)
    Per case, the largest (err - derived terms) / scale over its problems, output matrices and published row (one MI355X run; the
    same table with the classes: profiles/rows_matrix_notes.md):
        x2-k256-3slab-relu 6.1e-08, x2-k176-ragged-waves 4.4e-08, x2gn-k256-2x128-gs4 1.6e-07, x2gn-k256-2x128-gs8 1.4e-07,
        x2gn-k256-2x128-gs16 1.2e-07, x2gn-k176-gs16-ragged-waves 4.2e-08, x2gn-const-group 6.9e-08, x2gn-ratio64 0.0e+00,
        x2gn-nosilu-const-group 4.1e-08, x2gn-nosilu-ratio64 0.0e+00, x4gn-nosilu-gs32-ratio64 0.0e+00, x4-k512-4slab 3.2e-08,
        x4-k272 5.0e-08, x4gn-k384-gs32 4.5e-08, x4gn-plain-gn-plain-half 7.4e-08, x4gn-k272-gs16 6.5e-08, x8-k1024-2slab 3.5e-08,
        x8-k656 2.8e-08, x12-k1536 3.2e-08, x12-k1296 3.3e-08, x12-k1040-and-16 1.0e-07, x4-k272-act-relu 3.3e-08,
        x4-k272-act-silu 3.7e-08, x4-k272-act-sigmoid 5.2e-08, x2-res1 6.3e-08, x2-res2 5.7e-08, x2-res3 7.8e-08, x2-res4 8.0e-08,
        x2-res5 5.7e-08, x2-res6 6.7e-08, x2-res-step 6.7e-08, x2-s3-one-kblock-each 1.2e-07, x2-s5-one-kblock-each 1.1e-07,
        x2-s6-one-kblock-each 1.2e-07, x2-grid-5460 1.8e-07, f0-grid-5466 2.1e-07, x8g-gather-direct-gather 8.3e-08,
        x8g-k176-2slab 7.0e-08, x8g-k656 3.4e-08, x12g-k1040 1.2e-07, x12g-k1296 2.8e-08, x8g3-of-three 8.1e-08, x8g3-k656-pair 4.6e-08,
        x12g3-of-three 1.2e-07, x12g3-pair 8.3e-08, f0-gather-3slab 9.3e-08, x2-3-pair 6.0e-08, x2-3-of-three-rider 1.2e-07,
        x2gn-3-pair 5.4e-08, x2gn-3-of-three-rider 9.8e-08, x4-3-pair 6.2e-08, x4-3-of-three-rider 6.9e-08, x4gn-3-pair 6.2e-08,
        x4gn-3-of-three-rider 6.1e-08, x8-3-pair 6.2e-08, x8-3-of-three-rider 5.5e-08, split-x12-member 8.7e-08,
        split-csr-member 5.3e-08, f0-group-no-member 9.3e-08, xln-k192 8.8e-08, xln-k512-2slab-noaffine 4.2e-08, xln-k272 7.5e-08,
        xln-const-row 5.4e-08, xln-ratio64 0.0e+00, xln-geglu-n48 3.4e-08, xln-nt2-geglu-n32 2.9e-08, xln2-k512-two-slices 7.5e-08,
        xln2-k352 9.2e-08, xlnattn-w128 1.7e-07, xlnattn-const-t0-row 2.2e-07, xlnattn-ratio64 9.2e-08, xlnattn-nt2-ratio64 7.1e-08,
        xlnattn-w512-2slab 2.1e-07, xlnattn-w272 1.8e-07, xlnattn-nt2-w128 1.7e-07, xlnattn-nt2-w272 1.6e-07, f0-ln-k1024 3.4e-08,
        f0-ln-k520 3.5e-08, f0-csr-mean-relu 5.7e-08, f0-csr-mean-slabs 5.1e-08, f0-csr-sum-relu 4.6e-08, f0-csr-sum-slabs 7.1e-08,
        f0-csr-wavg-relu 4.0e-08, f0-csr-wavg-slabs 5.9e-08, f0-silu-prologue-1slab 7.2e-08, f0-geglu-prologue-1slab 1.0e-07,
        f0-silu-prologue-2slab 9.3e-08, f0-geglu-prologue-2slab 1.2e-07, f0-silu-prologue-4slab 8.7e-08,
        f0-geglu-prologue-4slab 1.5e-07, f0-silu-prologue-8slab 9.2e-08, f0-geglu-prologue-8slab 1.5e-07, f0-batch3 7.6e-08,
        f0-k72 6.4e-08, f0-5slab 7.0e-08, f0-8slab 6.9e-08, f0-gn-8slab 2.9e-07, f0-res7 7.0e-08, x2-res6-res2-6 7.0e-08,
        f0-step-segment 6.8e-08, f0-straddle 1.2e-07, f0-geglu-epilogue 4.0e-08, f0-k1040-2slab 4.6e-08, f0-7-slices 2.1e-07,
        f0-jw13 4.6e-08, f0-gn-class8 5.7e-08, f0-gather-gn 1.1e-07, x2-k256 4.3e-08, x4-k512 3.0e-08, x8-k528 3.5e-08,
        x8-k1024 2.6e-08, x12-k1040 4.0e-08, f0-k528-3slab 5.1e-08, x4-k512-3slab 3.6e-08, x2-6slab 5.6e-08, F0-plain-1slab 6.3e-08,
        F0-gn-1slab 1.4e-07, F0-plain-2slab 5.0e-08, F0-gn-2slab 1.4e-07, F0-plain-4slab 5.2e-08, F0-gn-4slab 4.1e-07,
        F0-plain-8slab 6.4e-08, F0-gn-8slab 3.2e-07, F0-k1040-two-chunks 5.9e-08, F0-gn-gs32-const 0.0e+00, F0-gn-gs4-ratio64 0.0e+00,
        F0-ln-k192 6.8e-08, F0-ln-k512-2slab 3.1e-08, F0-ln-k1024-2slab 3.9e-08, F0-ln-const-row 6.8e-08, F0-ln-ratio64 0.0e+00,
        F0-lnnt2-k192 3.5e-08, F0-lnnt2-k272-2slab 3.0e-08, F0-lnnt2-k520 3.1e-08, F0-lnnt2-k1024-2slab 2.5e-08,
        F0-fused-pair-rider 7.2e-08, F0-fused-plain-1slab-pair 6.0e-08, F0-fused-gn-1slab-pair 6.9e-08,
        F0-fused-general-1slab-pair 1.1e-07, F0-fused-plain-1slab-rider 8.1e-08, F0-fused-gn-1slab-rider 7.2e-08,
        F0-fused-general-1slab-rider 1.4e-07, F0-fused-plain-2slab-pair 8.0e-08, F0-fused-gn-2slab-pair 7.5e-08,
        F0-fused-general-2slab-pair 8.7e-08, F0-fused-plain-2slab-rider 7.6e-08, F0-fused-gn-2slab-rider 8.4e-08,
        F0-fused-general-2slab-rider 1.1e-07, F0-fused-plain-4slab-pair 6.9e-08, F0-fused-gn-4slab-pair 1.1e-07,
        F0-fused-general-4slab-pair 9.3e-08, F0-fused-plain-4slab-rider 7.4e-08, F0-fused-gn-4slab-rider 8.3e-08,
        F0-fused-general-4slab-rider 1.3e-07, F0-fused-plain-8slab-pair 6.3e-08, F0-fused-gn-8slab-pair 1.2e-07,
        F0-fused-general-8slab-pair 8.8e-08, F0-fused-plain-8slab-rider 8.9e-08, F0-fused-gn-8slab-rider 1.3e-07,
        F0-fused-general-8slab-rider 1.3e-07, F0-fused-csr-pair 5.9e-08, F0-fused-csr-rider 6.4e-08, F0-u1-4slab 1.9e-07,
        F0-u1-gn-4slab-rider 5.3e-07, F0-u1-gn-1slab 2.4e-07, F0-u1-gn-2slab 6.3e-07, F0-u1-4slab-rider 2.1e-07, F0-u1-gn-4slab 5.4e-07,
        F0-u1-gn-1slab-rider 2.3e-07, F0-u1-gn-2slab-rider 2.5e-07, F0-no-u1-256-workgroups 1.2e-07, pf-plain-next 7.4e-08,
        pf-sliced-next 5.7e-08, pf-nt2-next 6.0e-08, pf-fewer-than-8-workgroups 5.5e-08, pf-next-on-family0 6.2e-08,
        F0-u1env-1slab 6.3e-08, F0-u1env-1slab-pair 6.7e-08, F0-u1env-2slab-rider 7.6e-08, F0-u1env-2slab 6.8e-08
  * degenerate statistics, one case per norm prologue and family.  A CONSTANT group / row c has variance 0 in exact arithmetic; the
    kernels form the mean from an fp32 sum of k values (k = gs, or the row), so mean = c (1 + e), |e| <= (k + 1) 2^-24, and rstd <=
    eps^-1/2: the prologue output is within |gamma| |c| (k + 1) 2^-24 / sqrt(eps) of beta.  |mean| / spread = r = 64: the statistics
    are two-pass (mean, then centred squares), so the centred values are off by (k + 1) 2^-24 r spreads and the variance by the
    square of that: the prologue output is off by |gamma| (k + 1) 2^-24 r (1 + |z|).  Both terms go through |W| and the activation's
    derivative bound into the bound of the output; the tests print how much of them was used.  The formed row: the degenerate
    statistics are those of t0 (first round).  Its sums are taken about each wave's own pivot p_w; a constant row c leaves a variance
    of at most 4 (c (k + 1) 2^-24)^2 where the exact one is 0, so rstd(t0) is off by that / (2 eps) relative; at |mean| = r spreads the
    terms S_w - n p_w and (x - p_w)^2 carry (k + 1) 2^-24 r spreads of error against sums of order one spread, the variance is off by
    at most 8 (k + 1) 2^-24 r relative and rstd(t0) by 4 (k + 1) 2^-24 r (k = 40: a lane's values, the lane swaps, the eight waves).
    The published row x moves by dx = |u| rstd(t0) x that, and the LayerNorm of a row moved by at most E = max |dx| moves by at most
    rstd(x) E (2 + |z|);
  * inputs that make a subtle error show at 1e-2 of scale or more: every slab of an operand has its own magnitude and mixed signs
    (relu(sum) != sum(relu), a lost or doubled slab shows), rows, k-blocks and column tiles differ in magnitude, every (row, group)
    has its own mean and spread (side_matrix_cases.gn_target), gamma / beta / bias are of order 1 with both signs;
  * exact equalities (torch.equal on the bits): a second run; the rows of the M = 37 launch against the same rows launched at M = 5
    and M = 16; every problem of a fused launch (folded riders, groups that split, the U1 variants) against the problem launched
    alone; an operand of several plain slabs against the launch on the single operand ((s0 + s1) + s2) ... formed in fp32 on the
    host; an NT = 2 launch (N = 32) against column tiles 0 and 1 of the NT = 1 launch (N = 48) on the same weight rows, both families;
    a launch with the prefetch wave (two-op plan) against the same op launched directly; an isolated CSR node pools to exactly zero
    (its output row is the bias, bit for bit)."""
import ctypes as C
import math
import os
import subprocess
import sys
import zlib

import pytest
import torch

import rows_matrix_cases as rm
import side_matrix_cases as sm

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
from guarded_buffers import GuardedInput, GuardedOutput

pytestmark = pytest.mark.gpu

# 4 x the largest measured err / scale of the class, one significant digit, rounded up (the docstring); never above the ceilings
S_BAR = {'plain': 9e-7, 'gn': 3e-6, 'ln': 9e-7, 'exp': 7e-7}
S_CEIL = {'plain': 1e-5, 'gn': 1e-4, 'ln': 1e-4, 'exp': 1e-4}
assert all(S_BAR[k] <= S_CEIL[k] for k in S_BAR)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda')


@pytest.fixture
def family():
    from echoscene_amd import hip
    L = hip.lib()
    was = L.es_rows_get_kernel_family()
    yield lambda f: L.es_rows_set_kernel_family(f)
    L.es_rows_set_kernel_family(was)


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _signs(n, g):
    return torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)


# ---- logical values of a problem (CPU fp32 tensors), independent of strides -------------------------------------------------------------------

def make_values(p, key):
    """name -> tensor.  a{s}: [nmat, ns, rows, cols] (nmat: step table x batch; cols: w, 2K for a GEGLU prologue, [t0 | u] = 2w for the
    formed row); w: [nbatch, N, K]; bias [nbatch, N]; res / res2: [nmat, ns, M, Nout]; gamma / beta; the index lists"""
    M, N, K = p['M'], p['N'], p['K']
    v = {}
    for s, sg in enumerate(p['segs']):
        g = _gen(key, 'a', s)
        w = sg['w']
        rows = M + 11 if sg['mode'] == rm.GATHER else rm.CSR_T if sg['mode'] >= rm.CSRMEAN else M
        cols = 2 * K if sg['pro'] == rm.PRO_GEGLU else 2 * w
        nmat = (rm.NSTEP if sg['step'] else 1) * p['nbatch']
        ns = max(sg['ns'], 1)
        t = torch.randn((nmat, rows, cols), generator=g)
        norm = sg['pro'] in (rm.PRO_GN, rm.PRO_GN_SILU, rm.PRO_LN, rm.PRO_LN_ATTN)
        if norm:
            gs = sg['gs'] if sg['pro'] in (rm.PRO_GN, rm.PRO_GN_SILU) else w
            G = w // gs
            mean, spread = torch.empty(rows, G), torch.empty(rows, G)
            for r in range(rows):
                for gi in range(G):
                    if sg['inputs'] == 'ratio':
                        mean[r, gi], spread[r, gi] = (64.0 if (r + gi) % 2 == 0 else -64.0), 1.0
                    else:
                        mean[r, gi], spread[r, gi] = sm.gn_target(r, gi)
            x = t[:, :, :w].reshape(nmat, rows, G, gs) * spread[None, :, :, None] + mean[None, :, :, None]
            if sg['inputs'] == 'const':
                if sg['pro'] in (rm.PRO_LN, rm.PRO_LN_ATTN):
                    x[:, 1] = 0.7                   # row 1, the whole row (the formed row: the whole t0 row)
                else:
                    x[:, :, 1 % G] = 0.7            # group 1 of every row
            t[:, :, :w] = x.reshape(nmat, rows, w)
        else:
            # rows and k-blocks differ in magnitude
            t = t * (0.5 + 0.25 * (torch.arange(cols) // 16 % 5))[None, None, :] * (1.0 + 0.1 * (torch.arange(rows) % 7))[None, :, None]
        # slabs: slab j >= 1 has its own magnitude and both signs, slab 0 is what is left of the target (formed in fp32)
        slabs = [t]
        for j in range(1, ns):
            if norm and sg['inputs'] != 'spread':
                sl = torch.zeros_like(t)            # (the degenerate statistics are a statement about the summed operand)
            else:
                sl = torch.randn((nmat, rows, cols), generator=g) * (0.9 / j)
            slabs.append(sl)
            slabs[0] = slabs[0] - sl
        v['a%d' % s] = torch.stack(slabs, 1).contiguous()
        if sg['mode'] == rm.GATHER:
            v['idx%d' % s] = torch.tensor(rm.gather_index(M, rows), dtype=torch.int32)
        if sg['mode'] >= rm.CSRMEAN:
            ptr, er, eo = rm.csr_entries(M, w)
            v['idx%d' % s], v['ent_row%d' % s], v['ent_off%d' % s] = (torch.tensor(x_ or [0], dtype=torch.int32) for x_ in (ptr, er, eo))
            if sg['mode'] == rm.CSRWAVG:
                v['ent_wt%d' % s] = 0.05 + 0.9 * torch.rand((rm.CSR_T, 2), generator=g)
        if sg['pro'] in (rm.PRO_GN, rm.PRO_GN_SILU, rm.PRO_LN) and sg['affine']:
            v['gamma%d' % s] = (0.5 + torch.rand(w, generator=g)) * _signs(w, g)
            v['beta%d' % s] = (0.05 + torch.rand(w, generator=g)) * _signs(w, g)
    g = _gen(key, 'w')
    W = torch.randn((p['nbatch'], N, K), generator=g) / math.sqrt(K)
    W = W * (0.5 + 0.5 * (torch.arange(N) // 16 % 3))[None, :, None] * (0.6 + 0.2 * (torch.arange(K) // 16 % 4))[None, None, :]
    v['w'] = W
    if p['bias']:
        v['bias'] = (0.2 + torch.rand((p['nbatch'], N), generator=g)) * _signs(N, g)[None]
    No = rm.nout(p)
    if rm.is_lnattn(p):
        v['res2'] = torch.randn((1, 1, M, p['segs'][0]['w']), generator=g) * 0.5
    else:
        for nm in ('res', 'res2'):
            if p[nm]:
                nmat = rm.NSTEP if (nm == 'res' and p['res_step']) else 1
                r = torch.randn((nmat, p[nm], M, No), generator=g)
                v[nm] = r * (1.0 / (1 + torch.arange(p[nm])))[None, :, None, None] * (1.0 + 0.3 * (torch.arange(M) % 3))[None, None, :, None]
    return v


def rows_of(p, v, M):
    """the values of the same problem with its first M rows only (gather tables, CSR sources and weights stay whole)"""
    out = dict(v)
    for s, sg in enumerate(p['segs']):
        if sg['mode'] == rm.DIRECT:
            out['a%d' % s] = v['a%d' % s][:, :, :M].contiguous()
        elif sg['mode'] == rm.GATHER:
            # a table of M + 11 rows again, indexed by the smaller problem's own map, holding the rows the full problem gathered
            old, a = v['idx%d' % s].long(), v['a%d' % s]
            idx = torch.tensor(rm.gather_index(M, M + 11), dtype=torch.int32)
            tab = torch.full((a.shape[0], a.shape[1], M + 11, a.shape[3]), 9.0)
            for m in range(M):
                tab[:, :, int(idx[m])] = a[:, :, int(old[m])]
            for m in range(M):
                assert torch.equal(tab[:, :, int(idx[m])], a[:, :, int(old[m])])
            out['idx%d' % s], out['a%d' % s] = idx, tab
        else:
            out['idx%d' % s] = v['idx%d' % s][:M + 1].contiguous()
    for nm in ('res', 'res2'):
        if nm in v:
            out[nm] = v[nm][:, :, :M].contiguous()
    return out


# ---- physical buffers ---------------------------------------------------------------------------------------------------------------------------

class Problem:
    """one problem on the device: guarded buffers laid out by rm.geometry(), its es_linear_args, and the fp64 reference"""

    def __init__(self, dev, p, v, S_out):
        self.p, self.v, self.dev, self.S = p, v, dev, S_out
        bufs, g = rm.geometry(p)
        self.g = g
        M, K = p['M'], p['K']
        self.inputs = {}
        nan = float('nan')
        for s, sg in enumerate(p['segs']):
            d = g['seg'][s]
            a = v['a%d' % s]                                      # [nmat, ns, rows, cols]
            rows = a.shape[2]
            rows_g = d['rows']
            assert rows <= rows_g or sg['mode'] == rm.GATHER
            ld, w = d['ld'], sg['w']
            mat_rows = max(rows, rows_g)
            nmat, ns = a.shape[0], a.shape[1]
            phys = torch.full((nmat, ns, mat_rows * ld + (d['mat'] - rows_g * ld)), nan)
            m = phys[:, :, :mat_rows * ld].view(nmat, ns, mat_rows, ld)
            if sg['pro'] == rm.PRO_GEGLU:
                m[:, :, :rows, :2 * K] = a
            elif sg['pro'] == rm.PRO_LN_ATTN:
                m[:, :, :rows, :w] = a[..., :w]
                m[:, :, :rows, d['gs']:d['gs'] + w] = a[..., w:]
            elif sg['mode'] >= rm.CSRMEAN:
                m[:, :, :rows, :w] = a[..., :w]                    # slot at column offset 0 ...
                m[:, :, :rows, w + 8:2 * w + 8] = a[..., w:]       # ... and at w + 8
            else:
                m[:, :, :rows, :w] = a[..., :w]
            # strides: slabs sstr apart inside one matrix set, sets step_stride (step tables) or a_bstride (batches) apart
            if sg['step'] or sg['ns'] > 1:
                set_stride = d['step_stride']
                flat = torch.full((nmat * set_stride,), nan)
                for i in range(nmat):
                    for j in range(ns):
                        o = i * set_stride + j * d['sstr']
                        flat[o:o + phys.shape[2]] = phys[i, j]
            else:
                flat = phys[:, 0].reshape(-1)
            self.inputs['a%d' % s] = GuardedInput(dev, flat, torch.float32, 4096)
        for name, t in v.items():
            if name.startswith(('idx', 'ent_row', 'ent_off')):
                self.inputs[name] = _GuardedInts(dev, t)
            elif name.startswith(('gamma', 'beta', 'ent_wt')):
                self.inputs[name] = GuardedInput(dev, t.reshape(-1), torch.float32, 1024)
        if 'step' in bufs:
            self.inputs['step'] = _GuardedInts(dev, torch.tensor([rm.STEP], dtype=torch.int32))
        from echoscene_amd import hip
        L = hip.lib()
        N = p['N']
        wf = torch.empty(p['nbatch'] * g['wfloats'])
        for z in range(p['nbatch']):
            Wz = v['w'][z].contiguous()
            assert L.es_pack_linear_f32(C.c_void_p(Wz.data_ptr()), N, K, C.c_void_p(wf[z * g['wfloats']:].data_ptr())) == 0
        self.inputs['w'] = GuardedInput(dev, wf, torch.float32, 4096)
        if p['bias']:
            self.inputs['bias'] = GuardedInput(dev, v['bias'].reshape(-1), torch.float32, 1024)
        No = rm.nout(p)
        self.pub = None
        if rm.is_lnattn(p):
            w = p['segs'][0]['w']
            self.pub = GuardedOutput(dev, M, g['res_ld'], torch.float32)
            r2 = torch.full((M, g['res2_ld']), nan)
            r2[:, :w] = v['res2'][0, 0]
            self.inputs['res2'] = GuardedInput(dev, r2.reshape(-1), torch.float32, 1024)
        else:
            for nm, ld, sstr in (('res', g['res_ld'], g.get('res_sstr')), ('res2', g['res2_ld'], g.get('res2_sstr'))):
                if nm not in v:
                    continue
                r = v[nm]
                nmat, ns = r.shape[0], r.shape[1]
                set_stride = g['res_step_stride'] if nmat > 1 else ns * sstr
                flat = torch.full((nmat * set_stride,), nan)
                for i in range(nmat):
                    for j in range(ns):
                        mm = torch.full((M, ld), nan)
                        mm[:, :No] = r[i, j]
                        o = i * set_stride + j * sstr
                        flat[o:o + M * ld] = mm.reshape(-1)
                self.inputs[nm] = GuardedInput(dev, flat, torch.float32, 1024)
        # the output: S slabs (or nbatch batches) of M + 2 rows, out_ld = Nout + 8 columns, all NaN
        self.nmat_out = max(S_out, p['nbatch'])
        self.out = GuardedOutput(dev, self.nmat_out * (M + 2), g['out_ld'], torch.float32)
        addr = {k: b.view.data_ptr() for k, b in self.inputs.items()}
        addr['out'] = self.out.view.data_ptr()
        if self.pub is not None:
            addr['res'] = self.pub.view.data_ptr()
        self.args = rm.make_args(p, addr)
        self._assert_extents()

    def _assert_extents(self):
        """before anything runs: the last element that the argument struct lets a launch address lies inside its buffer"""
        a, p, v = self.args, self.p, self.v
        M, nb = p['M'], p['nbatch']
        for s, sg in enumerate(p['segs']):
            q, w = a.seg[s], sg['w']
            if sg['mode'] == rm.GATHER:
                rows = int(v['idx%d' % s].max()) + 1
            elif sg['mode'] >= rm.CSRMEAN:
                rows = int(v['ent_row%d' % s].max()) + 1
                assert int(v['idx%d' % s].max()) <= v['ent_row%d' % s].numel() and v['idx%d' % s].numel() == M + 1
            else:
                rows = M
            cols = 2 * p['K'] if sg['pro'] == rm.PRO_GEGLU else q.gs + w if sg['pro'] == rm.PRO_LN_ATTN else \
                (int(v['ent_off%d' % s].max()) + w) if sg['mode'] >= rm.CSRMEAN else w
            last = (max(q.nslab, 1) - 1) * q.slab_stride + (rm.NSTEP - 1) * q.step_stride * bool(q.step) + (nb - 1) * a.a_bstride + (rows - 1) * q.ld + cols
            assert last <= self.inputs['a%d' % s].view.numel(), (s, last, self.inputs['a%d' % s].view.numel())
            assert q.ptr == self.inputs['a%d' % s].view.data_ptr()
        No = rm.nout(p)
        assert self.inputs['w'].view.numel() == nb * ((p['N'] + 15) // 16) * ((p['K'] + 15) // 16) * 256
        assert not a.bias or self.inputs['bias'].view.numel() == nb * p['N']
        assert (self.S - 1) * a.out_slab_stride * (self.S > 1) + (nb - 1) * a.out_bstride + (M - 1) * a.out_ld + No <= self.out.view.numel()
        if self.pub is not None:
            wd = p['segs'][0]['w']
            assert (M - 1) * a.res_ld + wd <= self.pub.view.numel() and (M - 1) * a.res2_ld + wd <= self.inputs['res2'].view.numel()
        else:
            for nm, ptr, ld, ns, ss in (('res', a.res, a.res_ld, a.res_nslab, a.res_slab_stride), ('res2', a.res2, a.res2_ld, a.res2_nslab, a.res2_slab_stride)):
                if ptr:
                    last = (max(ns, 1) - 1) * ss + (rm.NSTEP - 1) * a.res_step_stride * bool(a.res_step and nm == 'res') + (M - 1) * ld + No
                    assert last <= self.inputs[nm].view.numel(), (nm, last)

    def result(self):
        """[nmat_out, M, Nout] of what was written"""
        M, No = self.p['M'], rm.nout(self.p)
        return self.out.view.view(self.nmat_out, M + 2, -1)[:, :M, :No].clone()

    def refill(self):
        self.out.refill()
        if self.pub is not None:
            self.pub.refill()

    def findings(self, tag):
        bad = []
        M, No = self.p['M'], rm.nout(self.p)
        for nm, b in self.inputs.items():
            if not b.unchanged():
                bad.append('%s: input %s (or its guards) was written' % (tag, nm))
        outs = [('out', self.out, self.out.view.view(self.nmat_out, M + 2, -1), No)]
        if self.pub is not None:
            outs.append(('the published row', self.pub, self.pub.view.view(1, M, -1), self.p['segs'][0]['w']))
        for nm, o, view, ncol in outs:
            if not o.guards_unchanged():
                bad.append('%s: the guard rows of %s were written' % (tag, nm))
            inside = torch.zeros_like(view, dtype=torch.bool)
            inside[:, :M, :ncol] = True
            fin = torch.isfinite(view)
            if bool((fin & ~inside).any()):
                bad.append('%s: %d elements of %s outside rows < M, columns < N were written' % (tag, int((fin & ~inside).sum()), nm))
            if bool((~fin & inside).any()):
                miss = (~fin & inside).nonzero()
                bad.append('%s: %s holds %d non-finite elements inside (never written, or computed from a guard): first at (slab %d, row %d, column %d)'
                           % (tag, nm, len(miss), *miss[0].tolist()))
        return bad

    # ---- fp64 ------------------------------------------------------------------------------------------------------------------------------
    def reference(self):
        """per output matrix (slab or batch): ref, bound-free pieces.  Returns lists over nmat_out of (ref, scale_pre, scale_res, extra_pre,
        act pieces) evaluated by `bound()`; and the published row's (ref, scale) for the formed row"""
        p, v = self.p, self.v
        M, N, K = p['M'], p['N'], p['K']
        eps = float(torch.tensor(p['eps'], dtype=torch.float32))
        out = []
        _, _, cuts = rm.slices_of(p)
        self.pub_ref = None
        for z in range(p['nbatch']):
            cols, extras = [], []
            for s, sg in enumerate(p['segs']):
                w = sg['w']
                a = v['a%d' % s].double()
                i = (rm.STEP if sg['step'] else 0) * p['nbatch'] + z
                full = a[i].sum(0) if a.shape[1] > 1 else a[i, 0]               # [rows, cols]: the slab sum
                relu = (lambda t: t.clamp(min=0)) if sg['relu'] else (lambda t: t)
                if sg['mode'] == rm.GATHER:
                    x = relu(full[v['idx%d' % s].long()][:, :w])
                elif sg['mode'] >= rm.CSRMEAN:
                    ptr, er, eo = (v[n_ + str(s)].tolist() for n_ in ('idx', 'ent_row', 'ent_off'))
                    x = torch.zeros(M, w, dtype=torch.float64)
                    for m in range(M):
                        acc, wsum = torch.zeros(w, dtype=torch.float64), 0.0
                        for e in range(ptr[m], ptr[m + 1]):
                            val = relu(full[er[e], :w] if eo[e] == 0 else full[er[e], w:2 * w])
                            wt = 1.0
                            if sg['mode'] == rm.CSRWAVG:
                                wt = float(v['ent_wt%d' % s][er[e], 1 if eo[e] else 0])
                                wsum += wt
                            acc += wt * val
                        den = max(ptr[m + 1] - ptr[m], 1) if sg['mode'] == rm.CSRMEAN else (wsum + float(torch.tensor(0.0001, dtype=torch.float32))) \
                            if sg['mode'] == rm.CSRWAVG else 1.0
                        x[m] = acc / den
                else:
                    x = relu(full[:M, :w])
                extra = torch.zeros(M, w, dtype=torch.float64)
                if sg['pro'] == rm.PRO_SILU:
                    x = x * torch.sigmoid(x)
                elif sg['pro'] == rm.PRO_GEGLU:
                    gate = relu(full[:M, K:2 * K])
                    x = x * 0.5 * gate * (1.0 + torch.erf(gate / math.sqrt(2.0)))
                elif sg['pro'] in (rm.PRO_GN, rm.PRO_GN_SILU, rm.PRO_LN):
                    gs = sg['gs'] if sg['pro'] != rm.PRO_LN else w
                    xg = x.view(M, w // gs, gs)
                    mean = xg.mean(2, keepdim=True)
                    var = ((xg - mean) ** 2).mean(2, keepdim=True)
                    zz = ((xg - mean) / torch.sqrt(var + eps)).view(M, w)
                    ga = v['gamma%d' % s].double() if 'gamma%d' % s in v else torch.ones(w, dtype=torch.float64)
                    be = v['beta%d' % s].double() if 'beta%d' % s in v else torch.zeros(w, dtype=torch.float64)
                    kk = (gs if sg['pro'] != rm.PRO_LN else 40) + 1          # fp32 roundings in the mean (docstring; LayerNorm: at most 4 values x 8 blocks + the combining levels)
                    if sg['inputs'] == 'const':
                        const = (var.expand_as(xg) == 0).reshape(M, w)
                        extra = torch.where(const, ga.abs()[None] * 0.7 * kk * 2.0 ** -24 / math.sqrt(eps), extra)
                    if sg['inputs'] == 'ratio':
                        extra = ga.abs()[None] * kk * 2.0 ** -24 * 64.0 * (1.0 + zz.abs())
                    x = zz * ga[None] + be[None]
                    if sg['pro'] == rm.PRO_GN_SILU:
                        x = x * torch.sigmoid(x)
                        extra = extra * 1.1
                elif sg['pro'] == rm.PRO_LN_ATTN:
                    t0, u = full[:M, :w], full[:M, w:2 * w]
                    var0 = ((t0 - t0.mean(1, keepdim=True)) ** 2).mean(1, keepdim=True)
                    rstd0 = 1.0 / torch.sqrt(var0 + eps)
                    row = u * rstd0 + t0 + v['res2'][0, 0].double()
                    # the relative error of rstd(t0) under degenerate statistics (docstring), k = 40 roundings in a row's sums
                    kk, rel = 41, torch.zeros(M, 1, dtype=torch.float64)
                    if sg['inputs'] == 'const':
                        rel = torch.where(var0 == 0, torch.tensor(4.0 * (0.7 * kk * 2.0 ** -24) ** 2 / (2.0 * eps), dtype=torch.float64), rel)
                    if sg['inputs'] == 'ratio':
                        rel = torch.full((M, 1), 4.0 * kk * 2.0 ** -24 * 64.0, dtype=torch.float64)
                    dx = (u * rstd0).abs() * rel
                    self.pub_ref = (row, (u * rstd0).abs() + t0.abs() + v['res2'][0, 0].double().abs(), dx)
                    mean = row.mean(1, keepdim=True)
                    var = ((row - mean) ** 2).mean(1, keepdim=True)
                    x = (row - mean) / torch.sqrt(var + eps)
                    # a row moved by at most E = max |dx| moves its LayerNorm by at most rstd E (2 + |z|): mean and centred values by 2 E,
                    # the standard deviation (a norm of the centred row) by E
                    extra = dx.max(1, keepdim=True).values / torch.sqrt(var + eps) * (2.0 + x.abs())
                cols.append(x)
                extras.append(extra)
            A, E = torch.cat(cols, 1), torch.cat(extras, 1)
            W = v['w'][z].double()
            for si in range(self.S):
                c0, c1 = (cuts[si] * 16, min(cuts[si + 1] * 16, K)) if self.S > 1 else (0, K)
                pre = A[:, c0:c1] @ W[:, c0:c1].T
                scale = A[:, c0:c1].abs() @ W[:, c0:c1].abs().T
                extra = E[:, c0:c1] @ W[:, c0:c1].abs().T
                res_sum, res_abs = torch.zeros(M, rm.nout(p), dtype=torch.float64), torch.zeros(M, rm.nout(p), dtype=torch.float64)
                if si == 0:
                    if p['bias']:
                        pre = pre + v['bias'][z].double()[None]
                        scale = scale + v['bias'][z].double().abs()[None]
                    if not rm.is_lnattn(p):
                        for nm in ('res', 'res2'):
                            if nm in v:
                                r = v[nm][rm.STEP if (nm == 'res' and p['res_step']) else 0].double()
                                res_sum, res_abs = res_sum + r.sum(0), res_abs + r.abs().sum(0)
                out.append(self._activate(pre, scale, extra, res_sum, res_abs))
        return out

    def _activate(self, pre, scale, extra, res_sum, res_abs):
        """(ref, f) with bound(s) = f(s): the bound of the pre-activation value s * scale + extra carried through the activation"""
        act = self.p['act']
        if act == rm.ACT_GEGLU:
            N = self.p['N']
            idx = torch.arange(N // 2)
            vi, gi = idx // 8 * 16 + idx % 8, idx // 8 * 16 + 8 + idx % 8
            val, gate = pre[:, vi], pre[:, gi]
            gelu = 0.5 * gate * (1.0 + torch.erf(gate / math.sqrt(2.0)))
            ref = val * gelu + res_sum
            return ref, lambda s: gelu.abs() * (s * scale[:, vi] + extra[:, vi]) + 1.13 * val.abs() * (s * scale[:, gi] + extra[:, gi]) + \
                s * (val * gelu).abs() + s * res_abs
        if act == rm.ACT_RELU:
            ref, d = pre.clamp(min=0), 1.0
        elif act == rm.ACT_SILU:
            ref, d = pre * torch.sigmoid(pre), 1.1
        elif act == rm.ACT_SIGMOID:
            ref, d = torch.sigmoid(pre), 0.25
        else:
            ref, d = pre, 1.0
        return ref + res_sum, lambda s: d * (s * scale + extra) + s * (ref.abs() if act else 0.0) + s * res_abs


class _GuardedInts:
    """an int32 list between guards of a value no index may take (a stray read would index far outside every table: caught by the
    table's NaN guards only if small -- so the guards hold 0x7fffffff and the list is compared bit for bit afterwards)"""

    def __init__(self, dev, t):
        g = 64
        self.whole = torch.full((2 * g + t.numel(),), 0x7fffffff, dtype=torch.int32, device=dev)
        self.view = self.whole[g:g + t.numel()]
        self.view.copy_(t)
        self.before = self.whole.clone()

    def unchanged(self):
        return torch.equal(self.whole, self.before)


# ---- one launch call ------------------------------------------------------------------------------------------------------------------------------

def case_class(c):
    cls = 'plain'
    for p in c['probs']:
        pros = {sg['pro'] for sg in p['segs']}
        if p['act'] in (rm.ACT_SILU, rm.ACT_SIGMOID, rm.ACT_GEGLU) or pros & {rm.PRO_SILU, rm.PRO_GEGLU}:
            return 'exp'
        if pros & {rm.PRO_LN, rm.PRO_LN_ATTN}:
            cls = 'ln'
        elif pros & {rm.PRO_GN, rm.PRO_GN_SILU} and cls == 'plain':
            cls = 'gn'
    return cls


def _sync():
    """wait for the launch; a device error ends the whole run here: nothing more is started on a GPU that has faulted"""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit('device error after a rows launch, nothing more is run: %s' % e, returncode=3)


class Call:
    """the problems of one launch call on the device, routed"""

    def __init__(self, dev, probs, values, nxt=None):
        from echoscene_amd import hip
        self.L = hip.lib()
        self.probs = [Problem(dev, p, v, rm.slices_of(p)[0]) for p, v in zip(probs, values)]
        self.nxt = nxt
        self.route = rm.route_of(self.L, [q.args for q in self.probs], None if nxt is None else nxt.args)

    def run(self):
        from echoscene_amd import hip
        args = [q.args for q in self.probs]
        if len(args) == 1:
            hip.check(self.L.es_linear_rows_f32(C.byref(args[0]), hip.current_stream()), 'es_linear_rows_f32')
        else:
            arr = (C.POINTER(hip.LinearArgs) * len(args))(*[C.pointer(a) for a in args])
            hip.check(self.L.es_linear_rows_multi_f32(arr, len(args), hip.current_stream()), 'es_linear_rows_multi_f32')
        _sync()

    def run_plan(self):
        """this call and the next op as a two-op plan: the runtime hints each launch with the other (the plan wraps around)"""
        from echoscene_amd import hip
        from echoscene_amd.plan import Builder
        b = Builder(self.probs[0].dev)
        for q in (self.probs[0], self.nxt):
            op = hip.Op()
            op.kind = hip.OP_LINEAR
            op.u.linear = q.args
            b.ops.append(op)
        # what es_plan_run will do, from the op list alone (the grouping and hint rule of the runtime as make_rows_routes.plan_groups
        # states it): op 0 is launched alone with op 1 as its next op, and that launch carries the ninth wave
        import make_rows_routes as mk
        groups = mk.plan_groups(b, 'plan')
        assert len(groups) == 2 and len(groups[0][1]) == 1 and groups[0][2] is not None
        assert C.addressof(groups[0][2]) == C.addressof(b.ops[1].u.linear) and C.addressof(groups[1][2]) == C.addressof(b.ops[0].u.linear)
        hinted = rm.route_of(self.L, [b.ops[0].u.linear], b.ops[1].u.linear)
        assert hinted is not None and hinted[0]['block'] == (576 if self.route[0]['pf']['gx'] else 512) and hinted[0]['pf'] == self.route[0]['pf']
        plan = b.finish()
        plan.run()
        _sync()

    def findings(self, tag):
        return [m for i, q in enumerate(self.probs) for m in q.findings('%s [problem %d]' % (tag, i))]


def assert_route(c, route, L):
    assert route is not None, '%s: refused: %s' % (c['name'], L.es_last_error().decode())
    assert len(route) == len(c['route']), '%s: %d launches, the table says %d (not run)' % (c['name'], len(route), len(c['route']))
    for g, e in zip(route, c['route']):
        exp = rm.expected_launch(c, e)
        exp['pf'] = rm.expected_prefetch(c['next'], c['pf_nt']) if e.get('prefetch') else rm.NO_PREFETCH
        got = {k: g[k] for k in exp}
        assert got == exp, '%s: routed to %s; the table says %s (not run)' % (c['name'], got, exp)


def check_values(c, call, tag, used):
    bad = []
    cls = case_class(c)
    s = S_BAR[cls]
    for i, q in enumerate(call.probs):
        res = q.result().double().cpu()
        for k, (ref, bound) in enumerate(q.reference()):
            err = torch.nan_to_num((res[k] - ref).abs(), nan=float('inf'))
            b1 = bound(1.0) - bound(0.0)                                     # the scale the class number multiplies
            ratio = ((err - bound(0.0)).clamp(min=0) / b1.clamp(min=1e-300)).max().item()
            derived = bound(0.0).max().item()
            used[cls] = max(used.get(cls, 0.0), ratio)
            print('%s problem %d matrix %d: largest (err - derived terms) / scale = %.3e (class %s, bar %.0e)%s'
                  % (tag, i, k, ratio, cls, S_BAR[cls], '' if derived == 0 else '; largest err / derived term = %.3f' %
                     (err / bound(0.0).clamp(min=1e-300))[bound(0.0) > 0].max().item()))
            over = err - bound(s)
            if not bool((over <= 0).all()):
                wr, wc = divmod(int(over.argmax()), ref.shape[1])
                bad.append('%s problem %d matrix %d: %d elements beyond the bound, worst at row %d column %d: got %.8g, fp64 %.8g, bound %.3e'
                           % (tag, i, k, int((over > 0).sum()), wr, wc, res[k][wr, wc].item(), ref[wr, wc].item(), bound(s)[wr, wc].item()))
        if q.pub is not None:
            row, scale, dx = q.pub_ref
            got = q.pub.view[:, :row.shape[1]].double().cpu()
            err = torch.nan_to_num((got - row).abs(), nan=float('inf'))
            ratio = ((err - dx).clamp(min=0) / scale).max().item()
            used['ln'] = max(used.get('ln', 0.0), ratio)
            print('%s problem %d published row: largest (err - derived terms) / scale = %.3e%s' % (tag, i, ratio, '' if not dx.any() else
                  '; largest err / derived term = %.3f' % (err / dx.clamp(min=1e-300))[dx > 0].max().item()))
            if not bool((err <= s * scale + dx).all()):
                bad.append('%s problem %d: the published row is off by up to %.3e of its scale' % (tag, i, ratio))
    return bad


def bits(t):
    return t.view(torch.int32)


def run_case(dev, c, used=None):
    """everything of one case but the child-process part; returns the findings"""
    from echoscene_amd import hip
    L = hip.lib()
    used = {} if used is None else used
    tag = c['name']
    probs = c['probs']
    values = [make_values(p, (tag, i)) for i, p in enumerate(probs)]
    nxt = None
    if c['next'] is not None:
        nxt = Problem(dev, c['next'], make_values(c['next'], (tag, 'next')), rm.slices_of(c['next'])[0])
    call = Call(dev, probs, values, nxt)
    assert_route(c, call.route, L)
    call.run()
    bad = call.findings(tag)
    bad += check_values(c, call, tag, used)
    first = [q.result() for q in call.probs]
    pubs = [None if q.pub is None else q.pub.view.clone() for q in call.probs]
    # ---- a second run leaves the same bits
    for q in call.probs:
        q.refill()
    call.run()
    bad += call.findings(tag + ' [second run]')
    for i, q in enumerate(call.probs):
        if not torch.equal(bits(q.result()), bits(first[i])):
            bad.append('%s problem %d: a second run leaves other bits' % (tag, i))
    # ---- the prefetch wave changes nothing: the two-op plan against the direct launches
    if nxt is not None:
        alone = Call(dev, [c['next']], [make_values(c['next'], (tag, 'next'))])
        alone.run()
        for q in call.probs:
            q.refill()
        call.run_plan()
        bad += call.findings(tag + ' [two-op plan]') + nxt.findings(tag + ' [two-op plan, next op]')
        if not torch.equal(bits(call.probs[0].result()), bits(first[0])):
            bad.append('%s: the launch with the prefetch wave leaves other bits than the direct launch' % tag)
        if not torch.equal(bits(nxt.result()), bits(alone.probs[0].result())):
            bad.append('%s: the next op of the plan leaves other bits than its direct launch' % tag)
    # ---- every problem of a fused launch equals the problem launched alone
    if len(probs) > 1:
        for i, p in enumerate(probs):
            one = Call(dev, [p], [values[i]])
            assert one.route is not None
            one.run()
            bad += one.findings('%s [problem %d alone]' % (tag, i))
            same_family = one.route[0]['family'] == [g for g in call.route if g['first'] <= i < g['first'] + g['nprob']][0]['family']
            if same_family and not torch.equal(bits(one.probs[0].result()), bits(first[i])):
                bad.append('%s: problem %d of the fused launch differs from the problem launched alone (%d elements)'
                           % (tag, i, int((bits(one.probs[0].result()) != bits(first[i])).sum())))
            if not same_family and len(call.route) > 1:
                bad.append('%s: problem %d of a group that splits is on another family than alone' % (tag, i))
    # ---- a row's bits do not depend on M
    big = max(p['M'] for p in probs)
    if len(probs) == 1 and big >= 37 and probs[0]['nbatch'] == 1:
        p = probs[0]
        for M in (5, 16):
            pm = dict(p, M=M)
            small = Call(dev, [pm], [rows_of(p, values[0], M)])
            assert small.route is not None and small.route[0]['kernel'] == call.route[0]['kernel'], (tag, M)
            small.run()
            bad += small.findings('%s [M = %d]' % (tag, M))
            if not torch.equal(bits(small.probs[0].result()), bits(first[0][:, :M])):
                bad.append('%s: rows 0..%d launched alone (M = %d) differ from the same rows of the M = %d launch' % (tag, M - 1, M, p['M']))
            if pubs[0] is not None and not torch.equal(bits(small.probs[0].pub.view[:, :p['segs'][0]['w']]), bits(pubs[0][:M, :p['segs'][0]['w']])):
                bad.append('%s: the published row at M = %d differs' % (tag, M))
    # ---- slabs are summed in fixed order: the same launch on the single operand ((s0 + s1) + s2) ... formed in fp32 on the host
    if len(probs) == 1 and all(sg['pro'] == rm.PRO_NONE and sg['mode'] <= rm.GATHER for sg in probs[0]['segs']) and \
            any(sg['ns'] > 1 for sg in probs[0]['segs']):
        p = probs[0]
        p1 = dict(p, segs=[dict(sg, ns=1) for sg in p['segs']])
        v1 = dict(values[0])
        for s_, sg in enumerate(p['segs']):
            a = values[0]['a%d' % s_]
            acc = a[:, 0].clone()
            for j in range(1, a.shape[1]):
                acc = acc + a[:, j]                                    # fp32, left to right
            v1['a%d' % s_] = acc[:, None].contiguous()
        folded = Call(dev, [p1], [v1])
        assert folded.route is not None
        if folded.route[0]['family'] == call.route[0]['family']:
            folded.run()
            bad += folded.findings(tag + ' [slabs summed on the host]')
            if not torch.equal(bits(folded.probs[0].result()), bits(first[0])):
                bad.append('%s: the launch on the host-summed operand differs: the slabs are not summed ((s0 + s1) + s2) ... before the ReLU'
                           % tag)
    # ---- an isolated CSR node pools to exactly zero: its row is the bias
    for i, p in enumerate(probs):
        if p['segs'][0]['mode'] >= rm.CSRMEAN and len(p['segs']) == 1:
            ptr = values[i]['idx0'].tolist()
            want = values[i]['bias'][0].to(dev) if p['bias'] else torch.zeros(p['N'], device=dev)
            for m in range(p['M']):
                if ptr[m] == ptr[m + 1] and not torch.equal(bits(first[i][0, m]), bits(want)):
                    bad.append('%s: the isolated node %d does not pool to exactly zero' % (tag, m))
    return bad


@pytest.mark.parametrize('c', [c for c in rm.CASES if not c['env']], ids=lambda c: c['name'])
def test_rows_matrix(dev, family, c):
    family(c['family'])
    used = {}
    bad = run_case(dev, c, used)
    assert not bad, '%d findings:\n%s' % (len(bad), '\n'.join(bad))


@pytest.mark.parametrize('fam,name', [(1, 'xln-nt2-geglu-n32'), (1, 'xlnattn-nt2-w272'), (0, 'F0-lnnt2-k272-2slab'), (0, 'F0-lnnt2-k520')])
def test_two_column_tiles_per_workgroup_equal_one(dev, family, fam, name):
    """NT = 2 (N = 32: tiles 0 and 1 in one workgroup) against column tiles 0 and 1 of the NT = 1 launch (N = 48, an odd tile count)
    whose packed tiles hold the same weight rows: the same bits, for the LayerNorm and (family 1) the formed-row kernels.

    This pair found the one kernel bug of the matrix (profiles/rows_matrix_notes.md): k_rows_x<4,2,3,1,2> and <4,2,3,1,1> left
    different bits for the same row (136 of 592 elements, up to 4.8e-7 apart, each within 4.2e-8 of scale of fp64), because the
    compiler had contracted the product mean = tot * inv_k into the subtractions that use it in 12 places of one instantiation and
    8 of the other.  The mean is now a value in a register before anything uses it."""
    family(fam)
    bad = []
    c = rm.BY_NAME[name]
    p2 = c['probs'][0]
    p1 = dict(p2, N=48)
    v2 = make_values(p2, (name, 0))
    v1 = make_values(p1, (name, 'wide'))
    for k in v2:
        if k not in ('w', 'bias'):
            v1[k] = v2[k]
    v1['w'][:, :32], v1['bias'][:, :32] = v2['w'], v2['bias']
    two, one = Call(dev, [p2], [v2]), Call(dev, [p1], [v1])
    assert two.route is not None and one.route is not None
    nt_at = 4 if fam == 1 else 6
    assert two.route[0]['tparam'][nt_at] == 2 and one.route[0]['tparam'][nt_at] == 1, (two.route[0]['kernel'], one.route[0]['kernel'])
    two.run()
    one.run()
    bad += two.findings(name) + one.findings(name + ' [N = 48]')
    if not torch.equal(bits(two.probs[0].result()), bits(one.probs[0].result()[:, :, :16])):
        d = bits(two.probs[0].result()) != bits(one.probs[0].result()[:, :, :16])
        bad.append('%s: NT = 2 and NT = 1 leave different bits (%d of %d elements, largest difference %.3e)'
                   % (name, int(d.sum()), d.numel(), (two.probs[0].result() - one.probs[0].result()[:, :, :16]).abs().max().item()))
    assert not bad, '\n'.join(bad)


def test_switch_cases_in_one_child_process(dev, family):
    """the U1 variants that only ES_ROWS_U1=2 reaches (the switch is read once per process): ONE child pytest process under its own
    time limit runs this very test with the switch set, and there every case goes through run_case -- route, guards, fp64, and every
    problem against the problem launched alone, which is the U1 kernel against the ordinary one"""
    cases = [c for c in rm.CASES if c['env']]
    assert cases and all(c['env'] == {'ES_ROWS_U1': '2'} for c in cases)
    if os.environ.get('ES_ROWS_U1') == '2':
        bad = []
        for c in cases:
            family(c['family'])
            bad += run_case(dev, c)
        assert not bad, '\n'.join(bad)
        return
    here = os.path.abspath(__file__)
    try:
        out = subprocess.run([sys.executable, '-m', 'pytest', here, '-m', 'gpu', '-q', '-x', '-s', '-k', 'test_switch_cases_in_one_child_process'],
                             env=dict(os.environ, ES_ROWS_U1='2'), capture_output=True, text=True, timeout=300, cwd=os.path.dirname(os.path.dirname(here)))
    except subprocess.TimeoutExpired:
        pytest.exit('the child process of the U1 cases hung (300 s): nothing more is run', returncode=3)
    print(out.stdout[-3000:])
    if out.returncode in (3, 124, 134, 137, 139, -6, -9, -11):
        pytest.exit('the child process of the U1 cases ended on a device error, an abort or a fault (%d): nothing more is run\n%s'
                    % (out.returncode, out.stdout[-2000:]), returncode=3)
    assert out.returncode == 0 and '1 passed' in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]
