"""What every op of a plan reads and writes, as regions of the plan's buffers, and the checks that follow from it.

Input: the canonical form of tests/golden/make_vol_plans.py (a pointer is [buffer ordinal, byte offset]; the buffer table holds sizes,
dtypes and the scratch flag), extended by ``extend()`` with what the recorded file does not carry: the contents of the int32 index
tensors (a gathered / pooled LINEAR segment reads exactly the rows its index names), which buffers ``Builder.buf`` left uninitialised,
and the rows of the per-step tables.  Nothing here depends on an address.

A Region is (field, buffer, byte offset, rows, row width in bytes, pitch in bytes).  A write is ``full`` (the op stores every byte),
partial (``full=False``: its bytes count as read as well and never as "written") or ``internal`` (scratch the op fills and consumes
itself -- split-K slabs, GroupNorm partial sums, the stem's pooled map: a write for every hazard check, no read, and nothing a later
op may rely on).  Route-dependent extents come from the library's host-only queries (es_conv_route_of, es_groupnorm_route_of,
es_linear_rows_slices, the pack-size functions), never from a constant copied out of a kernel.

``FOOTPRINT[kind](f, ctx)`` -> (reads, writes); ``f``: the op's fields by name.  Each extent cites the header comment
(include/echoscene_hip.h, "h:") or the kernel line (echoscene_amd/csrc, "k:") it was read from."""
import ctypes as C
import os
import sys
from contextlib import contextmanager
from types import SimpleNamespace

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(HERE, 'golden'), os.path.join(ROOT, 'tools')):
    if p not in sys.path:
        sys.path.insert(0, p)

import make_vol_plans as mv      # noqa: E402

F32, F16, I32 = 4, 2, 4


class Region:
    __slots__ = ('field', 'buf', 'off', 'rows', 'width', 'pitch', 'full', 'internal')

    def __init__(self, field, ptr, rows, width, pitch=None, off=0, full=True, internal=False):
        self.field, self.buf, self.off = field, ptr[0], ptr[1] + off
        self.rows, self.width = int(rows), int(width)
        self.pitch = self.width if pitch is None else int(pitch)
        if self.rows > 1 and self.pitch == self.width:            # contiguous rows: one span
            self.rows, self.width, self.pitch = 1, self.rows * self.width, self.rows * self.width
        self.full, self.internal = full, internal

    @property
    def end(self):
        return self.off + (self.rows - 1) * self.pitch + self.width

    def spans(self):
        return [(self.off + r * self.pitch, self.off + r * self.pitch + self.width) for r in range(self.rows)]

    def __repr__(self):
        return '%s=[buf %d +%d, %d x %d B / %d]' % (self.field, self.buf, self.off, self.rows, self.width, self.pitch)


def regions_overlap(a, b):
    """two regions share a byte.  Bounding ranges first; two multi-row regions of one pitch are column blocks of one matrix when the
    DIFFERENCE of their starts says so (never an address modulo the pitch: tools/plan_dryrun.rects_overlap); anything else by spans"""
    if a.buf != b.buf or a.width <= 0 or b.width <= 0 or not (a.off < b.end and b.off < a.end):
        return False
    if a.rows == 1 and b.rows == 1:
        return True
    if a.rows > 1 and b.rows > 1 and a.pitch == b.pitch and a.width <= a.pitch and b.width <= a.pitch:
        d = (b.off - a.off) % a.pitch
        return not (d >= a.width and d + b.width <= a.pitch)
    one, many = (a, b) if a.rows == 1 else (b, a)
    if one.rows == 1:
        lo, hi = one.off, one.end
        r0 = max(0, (lo - many.off - many.width) // many.pitch)
        for r in range(r0, many.rows):
            s = many.off + r * many.pitch
            if s >= hi:
                return False
            if s + many.width > lo:
                return True
        return False
    sb = b.spans()
    return any(x0 < y1 and y0 < x1 for x0, x1 in a.spans() for y0, y1 in sb)


# ------------------------------------------------------------------------------------------------ the library's answers
def _fill(inst, it):
    """a ctypes struct from the canonical field values, in make_vol_plans.flatten's order; a pointer [buffer, offset] becomes a
    synthetic, 4 KiB-aligned address that no query dereferences"""
    for fname, ftype in inst._fields_:
        if issubclass(ftype, C.Array):
            arr = getattr(inst, fname)
            for i in range(ftype._length_):
                if issubclass(ftype._type_, C.Structure):
                    _fill(arr[i], it)
                else:
                    arr[i] = _val(next(it), ftype._type_)
        elif issubclass(ftype, C.Structure):
            _fill(getattr(inst, fname), it)
        else:
            setattr(inst, fname, _val(next(it), ftype))


def _val(v, ftype):
    if ftype is C.c_void_p:
        return None if v is None else ((v[0] + 1) << 40) + v[1]
    return v


def struct_of(kind, values):
    from echoscene_amd import hip
    member = mv.kind_members()[kind]
    inst = dict(hip._OpU._fields_)[member]()
    _fill(inst, iter(values))
    return inst


def conv_route(kind, values):
    from echoscene_amd import hip
    a, info = struct_of(kind, values), hip.ConvRouteInfo()
    if hip.lib().es_conv_route_of(C.byref(a), C.byref(info)) != 0:
        raise RuntimeError('es_conv_route_of: ' + hip.lib().es_last_error().decode())
    return info


def gn_route(kind, values):
    from echoscene_amd import hip
    a, info = struct_of(kind, values), hip.GNRouteInfo()
    if hip.lib().es_groupnorm_route_of(C.byref(a), C.byref(info)) != 0:
        raise RuntimeError('es_groupnorm_route_of: ' + hip.lib().es_last_error().decode())
    return info


def linear_slices(kind, values):
    from echoscene_amd import hip
    a, got = struct_of(kind, values), C.c_int(0)
    S = hip.lib().es_linear_rows_slices(C.byref(a), C.byref(got))
    if S < 1:
        raise RuntimeError('es_linear_rows_slices: ' + hip.lib().es_last_error().decode())
    return S


# ------------------------------------------------------------------------------------------------ one function per op kind
def _slabs(field, ptr, n, stride_f, rows, width, pitch, out, off=0, **kw):
    """h: es_seg.nslab -- the value is the sum over j < nslab of ptr[j * slab_stride + ...] (0 / 1: a plain tensor)"""
    for j in range(max(n, 1)):
        out.append(Region(field, ptr, rows, width, pitch, off=off + j * stride_f * F32, **kw))


def fp_linear(f, ctx):
    from echoscene_amd import hip
    R, W = [], []
    M, K, N, nseg, nb = f['M'], f['K'], f['N'], f['nseg'], max(f['nbatch'], 1)
    ln_attn = nseg == 1 and f['seg[0].pro'] == hip.PRO_LN_ATTN
    for s in range(nseg):
        g = lambda n: f['seg[%d].%s' % (s, n)]      # noqa: E731
        name, ptr, w, ld = 'seg[%d].ptr' % s, g('ptr'), g('width') * F32, g('ld') * F32
        blocks = [0]                                 # column blocks of the source row this segment reads
        if g('pro') == hip.PRO_GEGLU or f['prologue'] == hip.PRO_GEGLU:
            blocks.append(K * F32)                   # k: es_rows.hip stage_chunk "src + a.K + 4 * c4" -- the gate columns sit K behind the value
        if ln_attn:
            blocks.append(g('gs') * F32)             # h: ES_PRO_LN_ATTN "u = `gs` columns behind the segment's pointer, same slabs"
        steps = [0]
        if g('step'):                                # h: es_seg.step "ptr += (*step) * step_stride": every row of the schedule counts
            R.append(Region('seg[%d].step' % s, g('step'), 1, I32))
            steps = [t * g('step_stride') * F32 for t in range(ctx.n_steps)]
        batches = [z * f['a_bstride'] * F32 for z in range(nb)] if s == 0 else [0]      # h: "batch z uses seg[0].ptr + z*a_bstride"
        mode = g('mode')
        if mode == hip.SEG_DIRECT:                   # k: stage_chunk "rowoff = mc * sg.ld" (ld = 0: one row for all M)
            rows = [(0, M if ld else 1)]
        elif mode == hip.SEG_GATHER:                 # k: stage_chunk "rowoff = sg.idx[mc] * sg.ld": idx [M], exactly those rows
            R.append(Region('seg[%d].idx' % s, g('idx'), 1, M * I32))
            rows = [(r * ld, 1) for r in sorted(set(ctx.ints(g('idx'), M)))]
        else:                                        # k: stage_chunk CSR branch: idx [M + 1] row pointer, entries idx[0] .. idx[M]
            R.append(Region('seg[%d].idx' % s, g('idx'), 1, (M + 1) * I32))
            rp = ctx.ints(g('idx'), M + 1)
            e0, e1 = rp[0], rp[M]
            R.append(Region('seg[%d].ent_row' % s, g('ent_row'), 1, (e1 - e0) * I32, off=e0 * I32))
            R.append(Region('seg[%d].ent_off' % s, g('ent_off'), 1, (e1 - e0) * I32, off=e0 * I32))
            er, eo = ctx.ints(g('ent_row'), e1)[e0:], ctx.ints(g('ent_off'), e1)[e0:]
            rows = [(r * ld + o * F32, 1) for r, o in sorted(set(zip(er, eo)))]      # k: "off = ent_row[ee] * sg.ld + ent_off[ee]"
            if mode == hip.SEG_CSRWAVG:              # h: es_seg.ent_wt "[rows of the source, 2]", one of the two per entry
                R += [Region('seg[%d].ent_wt' % s, g('ent_wt'), 1, F32, off=(2 * r + (1 if o else 0)) * F32) for r, o in sorted(set(zip(er, eo)))]
        for st in steps:
            for bz in batches:
                for cb in blocks:
                    for roff, nrows in rows:
                        _slabs(name, ptr, g('nslab'), g('slab_stride'), nrows, w, ld if nrows > 1 else None, R, off=st + bz + cb + roff)
        for n in ('gamma', 'beta'):                  # h: es_seg "affine gamma/beta [width]"
            if g(n):
                R.append(Region('seg[%d].%s' % (s, n), g(n), 1, w))
    # h: es_pack_linear_f32_size "number of floats of the packed image of W[N,K]"; batched: "images of equal shape stored back to back"
    R.append(Region('wpack', f['wpack'], 1, hip.lib().es_pack_linear_f32_size(N, K) * F32 * nb))
    if f['bias']:
        R.append(Region('bias', f['bias'], 1, N * F32 * nb))          # h: "bias + z*N"
    for n in ('gamma', 'beta'):
        if f[n]:
            R.append(Region(n, f[n], 1, K * F32))                     # h: es_linear_args.gamma "[K] affine of the norm prologue"
    Nout = N // 2 if f['act'] == hip.ACT_GEGLU else N                 # h: "ES_ACT_GEGLU: [M, N/2]"
    rw = f['seg[0].width'] if ln_attn else Nout                       # h: ES_PRO_LN_ATTN: res / res2 are as wide as the formed row
    for n in ('res', 'res2'):
        if not f[n]:
            continue
        ld = f[n + '_ld'] * F32
        if n == 'res' and ln_attn:                   # h: ES_PRO_LN_ATTN "The launch's `res` is then an OUTPUT: x is written there"
            W.append(Region('res', f['res'], M, rw * F32, ld))
            continue
        steps = [0]
        if n == 'res' and f['res_step']:             # h: es_linear_args.res_step "res + (*res_step) * res_step_stride floats"
            R.append(Region('res_step', f['res_step'], 1, I32))
            steps = [t * f['res_step_stride'] * F32 for t in range(ctx.n_steps)]
        for st in steps:                             # k: es_rows.hip epilogue "a.res + m_e * a.res_ld + nres" (res_ld = 0: one row)
            _slabs(n, f[n], f[n + '_nslab'], f[n + '_slab_stride'], M if ld else 1, rw * F32, ld if ld else None, R, off=st)
    # h: es_linear_args.kb_per_slice "slice s writes its partial products to out + s * out_slab_stride"; the count is the library's
    S = linear_slices(ctx.kind, ctx.values) if f['kb_per_slice'] > 0 else 1
    for bz in range(nb):                             # h: "out + z*out_bstride"
        for j in range(S):
            W.append(Region('out', f['out'], M, Nout * F32, f['out_ld'] * F32, off=(bz * f['out_bstride'] + j * f['out_slab_stride']) * F32))
    return R, W


def _step_rw(f, R, W, writes):
    R.append(Region('step', f['step'], 1, I32))      # k: es_update.hip "const int st = *a.step"
    if writes:
        W.append(Region('step', f['step'], 1, I32))  # k: k_step_inc / the ONE_BLOCK kernel's "*a.step = st + 1"


def _update_common(f, ctx, R, W, n_tab):
    n = f['n'] * F32
    R.append(Region('x', f['x'], 1, n))              # h: es_update_args.x "[n] state, updated in place"
    W.append(Region('x', f['x'], 1, n))
    _slabs('eps', f['eps'], f['eps_nslab'], f['eps_slab_stride'], 1, n, None, R)        # h: "eps as a slab tensor"
    R.append(Region('coef', f['coef'], 1, n_tab * f['coef_stride'] * F32))             # h: "coef [n_steps][coef_stride]"
    if f['noise']:                                   # h: "noise + (*step)*noise_stride is this step's draw"
        R.append(Region('noise', f['noise'], n_tab, n, f['noise_stride'] * F32))
    _step_rw(f, R, W, f['inc_step'])


def fp_update(f, ctx):
    R, W = [], []
    _update_common(f, ctx, R, W, ctx.n_steps)
    return R, W


def fp_keep(f, ctx):
    """es_ddpm_update_keep / es_ddim_rows_update: every element of x is stored (a kept row gets the next q_sample or x0): a full write"""
    R, W = [], []
    nt = f['n_tab']
    _update_common(f, ctx, R, W, nt)
    if f['mask']:
        n = f['n'] * F32
        R.append(Region('x0', f['x0'], 1, n))                                        # h: es_ddpm_keep_args.x0 "[n]"
        R.append(Region('mask', f['mask'], 1, f['n'] // f['row'] * F32))             # h: "mask [n / row]"
        R.append(Region('keep_noise', f['keep_noise'], nt, n, f['keep_noise_stride'] * F32))     # h: "[n_tab][keep_noise_stride]"
        R.append(Region('tab', f['tab'], 1, nt * 2 * F32))                           # h: "tab [n_tab][2]"
    return R, W


def fp_blend(f, ctx):
    """k: k_ddim_blend "if (i >= a.n || a.mask[o] == 0.0f) return": rows with mask 0 are neither read nor written -- a partial write"""
    n = f['O'] * f['n'] * F32
    R = [Region('x0', f['x0'], 1, n), Region('mask', f['mask'], 1, f['O'] * F32), Region('step', f['step'], 1, I32),
         Region('noise', f['noise'], ctx.n_steps, n, f['noise_stride'] * F32),       # h: es_blend_args.noise "[n_steps][noise_stride]"
         Region('tab', f['tab'], 1, ctx.n_steps * 2 * F32)]                          # h: "tab [n_steps][2]"
    return R, [Region('x', f['x'], 1, n, full=False)]


def fp_blend_vox(f, ctx):
    """k: k_ddim_blend_vox: a lane with four zero mask values returns before any other access -- a partial write"""
    n = f['O'] * f['C'] * f['V'] * F32
    R = [Region('x0', f['x0'], 1, n), Region('mask', f['mask'], 1, f['O'] * f['V'] * F32), Region('step', f['step'], 1, I32),
         Region('noise', f['noise'], ctx.n_steps, n, f['noise_stride'] * F32), Region('tab', f['tab'], 1, ctx.n_steps * 2 * F32)]
    return R, [Region('x', f['x'], 1, n, full=False)]


def _plms(mode):
    def fp(f, ctx):
        n = f['n'] * F32
        R, W = [], [Region('x', f['x'], 1, n)]
        _slabs('eps', f['eps'], f['eps_nslab'], f['eps_slab_stride'], 1, n, None, R)
        if mode == 'update':                         # k: k_plms UPDATE: h1..h3 from the ring, slot st % 3 rewritten: which one the step decides
            R += [Region('x', f['x'], 1, n), Region('coef', f['coef'], 1, ctx.n_steps * f['coef_stride'] * F32),
                  Region('ring', f['ring'], 3, n, f['ring_stride'] * F32)]
            W.append(Region('ring', f['ring'], 3, n, f['ring_stride'] * F32, full=False))
            _step_rw(f, R, W, f['inc_step'])
        elif mode == 'first_a':                      # k: k_plms FIRST_A "xsave = x, ring[0] = e, x = ddim(x, e, coef row 0)", then k_step_set
            R += [Region('x', f['x'], 1, n), Region('coef', f['coef'], 1, f['coef_stride'] * F32)]
            W += [Region('xsave', f['xsave'], 1, n), Region('ring', f['ring'], 1, n), Region('step', f['step'], 1, I32)]
        else:                                        # k: k_plms FIRST_B "x = ddim(xsave, (ring[0] + e) / 2, coef row 0)"
            R += [Region('xsave', f['xsave'], 1, n), Region('ring', f['ring'], 1, n), Region('coef', f['coef'], 1, f['coef_stride'] * F32)]
        return R, W
    return fp


def fp_copy(f, ctx):
    """k: es_runtime.hip dispatch ES_OP_COPY: hipMemcpy2DAsync(rows x bytes with pitches) for rows > 1, else hipMemcpyAsync(bytes)"""
    rows = f['rows'] if f['rows'] > 1 else 1
    return ([Region('src', f['src'], rows, f['bytes'], f['src_pitch'] if rows > 1 else None)],
            [Region('dst', f['dst'], rows, f['bytes'], f['dst_pitch'] if rows > 1 else None)])


def _conv_in_grid(f):
    """h: es_conv_args.mode -- the input grid of an output grid (D, H, W)"""
    from echoscene_amd import hip
    D, H, W = f['D'], f['H'], f['W']
    return {hip.CONV_SAME: (D, H, W), hip.CONV_DOWN_HW: (D, 2 * H, 2 * W), hip.CONV_UP_HW: (D, H // 2, W // 2),
            hip.CONV_UP_DHW: (D // 2, H // 2, W // 2), hip.CONV_DOWN_DHW: (2 * D, 2 * H, 2 * W),
            hip.CONV_DOWN_DHW_P01: (2 * D, 2 * H, 2 * W)}[f['mode']]


def fp_conv(f, ctx):
    from echoscene_amd import hip
    L = hip.lib()
    f32 = ctx.kind == hip.OP_CONV_F32
    el = F32 if f32 else F16                          # h: "es_conv_f32 ... the same argument structs with fp32 activations"
    O, N, Cin, taps = f['O'], f['N'], f['Cin'], f['taps']
    V = f['D'] * f['H'] * f['W']
    M = O * V
    Di, Hi, Wi = _conv_in_grid(f)
    R = [Region('a', f['a'], 1, O * Di * Hi * Wi * Cin * el)]                 # h: es_conv_args.a "[O, D, Hi, Wi, Cin] (channels-last)"
    W = []
    info = None if f32 else conv_route(ctx.kind, ctx.values)
    if f32:                                          # h: es_pack_conv_f32 "fp32 weights ([N][taps][Cin16])"
        R.append(Region('w', f['w'], 1, L.es_pack_conv_f32_size(N, Cin, taps) * F32))
    elif N <= 4 and taps == 27 and Cin <= 64:        # h: es_conv_args.w "es_pack_conv_rows_f16 ([N][27][Cin])"
        R.append(Region('w', f['w'], 1, N * taps * Cin * F16))
    else:                                            # h: es_pack_conv_f16_size: the tiled image the kernel streams
        R.append(Region('w', f['w'], 1, L.es_pack_conv_f16_size(N, Cin, taps) * F16))
    if f['a2']:                                      # h: "optional second contraction ... the 1x1 skip_connection": a2 [M, Cin2], w2 a 1-tap image
        R.append(Region('a2', f['a2'], 1, M * f['Cin2'] * el))
        R.append(Region('w2', f['w2'], 1, (L.es_pack_conv_f32_size(N, f['Cin2'], 1) * F32) if f32 else L.es_pack_conv_f16_size(N, f['Cin2'], 1) * F16))
    elif f['w2'] and info is not None and hip.CONV_KERNELS[info.kernel] == 'ws_256_up_fold':
        # h: "w2 WITHOUT a2 ... the library multiplies through the folded image on one route only ... and ignores it on every other"
        R.append(Region('w2', f['w2'], 1, L.es_pack_conv_up_fold_f16_size(N, Cin) * F16))
    if f['bias']:
        R.append(Region('bias', f['bias'], 1, N * F32))                          # h: "bias [N]"
    if f['rowvec']:                                  # h: "rowvec [O, rowvec_ld] per-object vector broadcast over voxels" (ld 0: one row)
        ld = f['rowvec_ld'] * F32
        R.append(Region('rowvec', f['rowvec'], O if ld else 1, N * F32, ld if ld else None))
    ncdhw = f['out_ld'] < 0                          # h: "out_ld < 0: out_f32 is written as NCDHW [O, N, D*H*W]"
    pitch = None if ncdhw else f['out_ld'] * F32
    if f['res']:                                     # h: "res: fp32 residual [M, N]", out_ld "leading dimension of both outputs and of res"
        R.append(Region('res', f['res'], M, N * F32, pitch))
    geglu = f['epilogue'] == hip.EPI_GEGLU
    if f['out_f32']:
        W.append(Region('out_f32', f['out_f32'], M, N * F32, pitch))
    if f['out_f16']:                                 # h: ES_EPI_GEGLU "the only output is out_f16 [M, 4C]", N = 8C
        No = N // 2 if geglu else N
        W.append(Region('out_f16', f['out_f16'], M, No * el, None if ncdhw else f['out_ld'] * el))
    if info is not None:
        if info.reduce:                              # h: es_conv_split_of "the number of fp32 slabs [S][M][N] ... writes into args->workspace"
            W.append(Region('workspace', f['workspace'], 1, info.slabs * M * N * F32, internal=True))
        if f['gn_stats_out'] and (info.stats or info.stats_pass):     # h: gn_stats_out "[2][ceil(M/64)][N] fp32"
            W.append(Region('gn_stats_out', f['gn_stats_out'], 1, 2 * ((M + 63) // 64) * N * F32))
        if f['gn_part_out'] and info.reduce == 2:    # h: gn_part_out "[O][ntiles][gn_part_groups][2]", tiles of es_conv_route_info.vt voxels
            W.append(Region('gn_part_out', f['gn_part_out'], 1, O * ((V + info.vt - 1) // info.vt) * f['gn_part_groups'] * 2 * F32))
    return R, W


def fp_gn(f, ctx):
    from echoscene_amd import hip
    r = gn_route(ctx.kind, ctx.values)
    O, V, G, Cc = f['O'], f['V'], f['groups'], f['C1'] + f['C2']
    M = O * V
    R = [Region('x1', f['x1'], 1, M * f['C1'] * (F16 if f['x1_is_f16'] else F32)),       # h: es_gn_args.x1 "[O, V, C1]" (x1_is_f16: f16)
         Region('gamma', f['gamma'], 1, Cc * F32), Region('beta', f['beta'], 1, Cc * F32)]     # h: "gamma, beta [C1+C2]"
    if f['x2']:
        R.append(Region('x2', f['x2'], 1, M * f['C2'] * F32))
    W = []
    part = O * r.ntiles * G * 2 * F32                # k: es_vol.hip es_groupnorm_vol: k_gn_partial writes [O][ntiles][groups][2] at stats
    fin = O * G * 2 * F32                            # h: es_gn_route_info.fin_offset "the final [O][groups][2] statistics"
    if r.stats_src == hip.GN_STATS_SOURCES.index('pass'):
        W.append(Region('stats', f['stats'], 1, part, internal=True))
    elif r.stats_src == hip.GN_STATS_SOURCES.index('part_in'):      # h: es_gn_args.part_in "the partial sums the producing conv's split-K reduction left"
        R.append(Region('part_in', f['part_in'], 1, part))
    else:                                            # h: es_gn_args.stats1 "[2][O*V/64][C1] row-group sums", stats2 [2][O*V/64][C2]
        R.append(Region('stats1', f['stats1'], 1, 2 * (M // 64) * f['C1'] * F32))
        if f['x2']:
            R.append(Region('stats2', f['stats2'], 1, 2 * (M // 64) * f['C2'] * F32))
    if r.fin_offset >= 0:                            # k: es_groupnorm_vol "fin = a->stats + r.fin_off" (k_gn_finalize / k_gn_finalize_rg write, k_gn_apply reads)
        W.append(Region('stats', f['stats'], 1, fin, off=r.fin_offset * F32, internal=True))
    el = F32 if f['y_is_f32'] else F16               # h: "y_is_f32: y_f16 / raw_f16 point at FP32 tensors"
    W.append(Region('y_f16', f['y_f16'], 1, M * Cc * el))
    if f['raw_f16']:
        W.append(Region('raw_f16', f['raw_f16'], 1, M * Cc * el))
    return R, W


def fp_ln(f, ctx):
    n = f['M'] * f['C']                              # h: es_ln_args: x [M, C], gamma / beta [C], y [M, C] (y_is_f32: fp32)
    return ([Region('x', f['x'], 1, n * F32), Region('gamma', f['gamma'], 1, f['C'] * F32), Region('beta', f['beta'], 1, f['C'] * F32)],
            [Region('y_f16', f['y_f16'], 1, n * (F32 if f['y_is_f32'] else F16))])


def fp_attn(f, ctx):
    from echoscene_amd import hip
    el = F32 if ctx.kind == hip.OP_ATTN_F32 else F16          # h: "qkv / out of es_attention_f32 are fp32"
    rows, Cc = f['B'] * f['Ntok'], f['heads'] * f['dhead']    # h: es_attn_args.qkv "[B*Ntok, 3*C]", out_f16 "[B*Ntok, C]"
    return [Region('qkv', f['qkv'], 1, rows * 3 * Cc * el)], [Region('out_f16', f['out_f16'], 1, rows * Cc * el)]


def fp_geglu(f, ctx):                                # h: es_geglu_args "h: [M, 2*C4] value|gate; out_is_f32: fp32 result"
    return ([Region('h_f32', f['h_f32'], 1, f['M'] * 2 * f['C4'] * F32)],
            [Region('out_f16', f['out_f16'], 1, f['M'] * f['C4'] * (F32 if f['out_is_f32'] else F16))])


def fp_tocl(f, ctx):
    O, Cc, V, Cp = f['O'], f['C'], f['V'], f['Cpad']
    if f['out_is_f32'] == 2:                         # h: es_tocl_args "x is channels-last fp32 [O * V, C] ... out ... f16 [O * V, 3 C]" (k: k_split_f16x3)
        return [Region('x', f['x'], 1, O * V * Cc * F32)], [Region('out', f['out'], 1, O * V * 3 * Cc * F16)]
    # k: k_to_cl: every one of the O * V * Cpad outputs is stored (zero in the padding channels)
    return [Region('x', f['x'], 1, O * Cc * V * F32)], [Region('out', f['out'], 1, O * V * Cp * (F32 if f['out_is_f32'] else F16))]


def fp_stem(f, ctx):
    O, Cx = f['O'], f['Cin'] or 3                    # h: es_stem_args.Cin "0 = 3"
    ost = (f['x_ostride'] or Cx * 4096) * F32        # h: "x_ostride: floats between objects in x; 0 = Cin * 4096"
    R = [Region('x', f['x'], O, Cx * 4096 * F32, ost),
         Region('w0', f['w0'], 1, 32 * Cx * 27 * F32), Region('b0', f['b0'], 1, 32 * F32),        # h: "Conv3d(3,32,3) weights [32,3,3,3,3]"
         Region('w1', f['w1'], 1, 64 * 32 * 27 * F32), Region('b1', f['b1'], 1, 64 * F32)]        # h: "Conv3d(32,64,3) weights [64,32,3,3,3]"
    # h: es_stem_args.scratch "[O,32,8,8,8] pooled stage-1 output" (k_stem1 writes, k_stem2 reads); out "[O,512]"
    return R, [Region('scratch', f['scratch'], 1, O * 32 * 512 * F32, internal=True), Region('out', f['out'], 1, O * 512 * F32)]


def fp_vq(f, ctx):
    M = f['O'] * f['V']                              # h: es_vq_args: z [O,3,V], codebook / lut [n_embed,3], idx_out [O*V], out_f16 [O*V, Cpad]
    R = [Region('z', f['z'], 1, 3 * M * F32), Region('codebook', f['codebook'], 1, f['n_embed'] * 3 * F32),
         Region('lut', f['lut'], 1, f['n_embed'] * 3 * F32)]
    W = [Region('out_f16', f['out_f16'], 1, M * f['Cpad'] * F16)]       # k: k_vq_lookup stores all Cpad columns (zero past 3)
    if f['idx_out']:
        W.append(Region('idx_out', f['idx_out'], 1, M * I32))
    return R, W


def fp_rowsel(f, ctx):
    """k: k_row_select "a.table[(*a.step) * a.stride + i]" for i < n; out[r * out_ld + i] for r < rows"""
    return ([Region('table', f['table'], ctx.n_steps, f['n'] * F32, f['stride'] * F32), Region('step', f['step'], 1, I32)],
            [Region('out', f['out'], f['rows'], f['n'] * F32, f['out_ld'] * F32)])


def fp_conv_c1(f, ctx):
    M = f['O'] * f['D'] * f['H'] * f['W']            # h: es_conv_c1_args: x [O, D, H, W], w [N][27], bias [N], out [O*D*H*W, N]
    R = [Region('x', f['x'], 1, M * F32), Region('w', f['w'], 1, f['N'] * 27 * F32)]
    if f['bias']:
        R.append(Region('bias', f['bias'], 1, f['N'] * F32))
    W = [Region(n, f[n], 1, M * f['N'] * el) for n, el in (('out_f32', F32), ('out_f16', F16)) if f[n]]
    return R, W


def footprint_table():
    from echoscene_amd import hip as h
    return {h.OP_LINEAR: fp_linear, h.OP_DDPM: fp_update, h.OP_DDIM: fp_update, h.OP_COPY: fp_copy, h.OP_CONV: fp_conv, h.OP_GN: fp_gn,
            h.OP_LN: fp_ln, h.OP_ATTN: fp_attn, h.OP_GEGLU: fp_geglu, h.OP_TO_CL: fp_tocl, h.OP_STEM: fp_stem, h.OP_VQ: fp_vq,
            h.OP_ROWSEL: fp_rowsel, h.OP_CONV_F32: fp_conv, h.OP_ATTN_F32: fp_attn, h.OP_DDIM_BLEND: fp_blend, h.OP_CONV_C1: fp_conv_c1,
            h.OP_DDPM_KEEP: fp_keep, h.OP_PLMS: _plms('update'), h.OP_PLMS_FIRST_A: _plms('first_a'), h.OP_PLMS_FIRST_B: _plms('first_b'),
            h.OP_DDIM_ROWS: fp_keep, h.OP_DDIM_BLEND_VOX: fp_blend_vox, h.OP_FORK: None, h.OP_JOIN: None}


def aliasing_ok():
    """kind -> {(written field, read field): reason}: the only overlaps of a write with a read of the SAME op that are no finding"""
    from echoscene_amd import hip as h
    inplace = {('x', 'x'): 'the update rewrites x element-wise in place: a lane reads x[i] and stores x[i] (es_update.hip)',
               ('step', 'step'): 'the step counter is advanced after every lane has read it (k_step_inc / the one-block kernel)'}
    ring = dict(inplace)
    ring[('ring', 'ring')] = 'k_plms reads h1..h3 and rewrites slot st % 3 of the same lane ("read before the slot is overwritten")'
    return {h.OP_DDPM: inplace, h.OP_DDIM: inplace, h.OP_DDPM_KEEP: inplace, h.OP_DDIM_ROWS: inplace, h.OP_PLMS: ring,
            h.OP_PLMS_FIRST_A: {('x', 'x'): inplace[('x', 'x')]}}


KIND_NAMES = {}


def kind_name(k):
    if not KIND_NAMES:
        from echoscene_amd import hip
        KIND_NAMES.update({v: n[3:] for n, v in vars(hip).items() if n.startswith('OP_')})
    return KIND_NAMES.get(k, 'kind %d' % k)


# ------------------------------------------------------------------------------------------------ the extended canonical form
@contextmanager
def recording_allocations(log):
    """while active, every Builder.buf call is noted in ``log`` as (data_ptr, zero, scratch): the canonical form keeps the scratch flag
    only, and "written before read" also has to hold for the other torch.empty buffers"""
    from echoscene_amd import plan
    orig = plan.Builder.buf

    def buf(self, *shape, dtype=None, zero=False, scratch=False):
        t = orig(self, *shape, zero=zero, scratch=scratch, **({} if dtype is None else dict(dtype=dtype)))
        log.append((t.data_ptr(), bool(zero), bool(scratch)))
        return t
    plan.Builder.buf = buf
    try:
        yield log
    finally:
        plan.Builder.buf = orig


def _int_tensors(roots):
    """storage start -> flat int list, of the integer tensors reachable from the roots (make_vol_plans.Buffers' walk)"""
    import torch
    found, seen = {}, set()

    def walk(o):
        if o is None or id(o) in seen:
            return
        seen.add(id(o))
        if isinstance(o, torch.Tensor):
            if o.dtype in (torch.int32, torch.int64) and o.numel():
                st = o.untyped_storage()
                if st.data_ptr() not in found:
                    found[st.data_ptr()] = (o.dtype, st)
        elif isinstance(o, (list, tuple, set)):
            for v in o:
                walk(v)
        elif isinstance(o, dict):
            for v in o.values():
                walk(v)
        elif hasattr(o, '__dict__') and type(o).__module__.startswith('echoscene_amd'):
            walk(vars(o))
    walk(roots)
    out = {}
    for start, (dt, st) in found.items():
        out[start] = torch.tensor([], dtype=dt, device=st.device).set_(st).cpu().tolist()
    return out


def extend(b, roots, out=None, allocations=(), n_steps=4):
    """make_vol_plans.canonical(b, roots, out) + 'ints' {buffer ordinal: contents of an integer tensor}, 'empty' [ordinals of the
    buffers Builder.buf left uninitialised and unclaimed], 'n_steps' (rows of the per-step tables)"""
    bufs = mv.Buffers([b.keep, roots, out], set(b.scratch))
    doc = dict(ops=[mv.canon_op(op, bufs, 'op %d' % i) for i, op in enumerate(b.ops)])
    first = (out or {}).get('first_ops', (None, None))
    doc['first_ops'] = [None if op is None else mv.canon_op(op, bufs, 'first op %d' % i) for i, op in enumerate(first)]
    doc['tags'] = {n: bufs.ref(b.tags[n].ptr, 'tag ' + n) for n in sorted(b.tags)}
    if out is not None:
        doc['values'] = {k: (list(out[k]) if isinstance(out[k], tuple) else out[k]) for k in mv.RESULT_VALUES}
        doc['tensors'] = {k: None if out.get(k) is None else [list(out[k].shape), bufs.ref(out[k].data_ptr(), k)] for k in mv.RESULT_TENSORS}
    doc['buffers'] = bufs.table()
    ints = _int_tensors([b.keep, roots, out])
    doc['ints'] = {bufs.ordinal[s]: v for s, v in ints.items() if s in bufs.ordinal}
    doc['empty'] = sorted(bufs.ordinal[p] for p, zero, scratch in allocations if not zero and not scratch and p in bufs.ordinal)
    doc['n_steps'] = n_steps
    doc['starts'] = list(bufs.order)                 # (addresses: for the GPU witness only, never compared)
    return doc


def emit_extended(name):
    """the extended document of a configuration of make_vol_plans.CONFIGS (emitted on the CPU Builder)"""
    log = []
    with recording_allocations(log):
        b, roots, out = mv.emit(name)
    return extend(b, roots, out, log)


def tensor_region(doc, name, cols=None):
    """the region of a result tensor of the document (``cols``: its first columns only), as a full write in front of the replay"""
    shape, ptr = doc['tensors'][name]
    rows, row = shape[0], 1
    for d in shape[1:]:
        row *= d
    return Region(name, ptr, rows, (row if cols is None else cols) * F32, row * F32)


# What the caller of emit_shape_step fills before a replay (samplers.ShapeDenoiser): the latents x; the conditioning columns of objbuf
# (plan_vol.emit_unet3d_step "objbuf[:, :ucw].copy_(uc_dev)", ShapeDenoiser "st['objbuf'][:, :st['ucw']].copy_").  Everything else
# that Builder.buf left uninitialised has to be written by the plan before it is read.
# 'concat': channel 3 of the staging tensor xc, c_s ("xc[:, 3].copy_(c_dev)  # constant over the loop: written once at plan build");
# without message passing the conditioning cdev ("refreshed by the caller for every sample"); eta != 0: the per-step draws snoise.
# The layout step (samplers.emit_layout_step): x and the embedding columns of objbuf ("st['objbuf'][:, :st['oe_w']].copy_").
def step_inputs(doc):
    t = doc['tensors']
    inputs = [tensor_region(doc, 'x')]
    if t.get('objbuf'):
        inputs.append(tensor_region(doc, 'objbuf', cols=doc['values']['ucw']))
    if t.get('xc'):
        shape, ptr = t['xc']
        inputs.append(Region('xc', ptr, shape[0], shape[2] * F32, shape[1] * shape[2] * F32, off=3 * shape[2] * F32))
    for n in ('cdev', 'snoise'):
        if t.get(n):
            inputs.append(tensor_region(doc, n))
    return inputs


# The VQ plans (plan_vol.emit_vq_decode / emit_vq_encode): the caller's input is what the first op reads -- the latents z of
# es_vq_lookup, the volume x of es_conv_c1_f32.
VQ_INPUT_FIELD = {'vq decode': 'z', 'vq encode fp16': 'x'}


def vq_inputs(name, doc):
    R, _ = op_footprint(doc, doc['ops'][0])
    return [g for g in R if g.field == VQ_INPUT_FIELD[name]]


# The configurations tests/test_hip_plan_footprint.py runs on the device: the smallest set that holds every op kind, every GroupNorm
# statistics source and every conv route class of all the others (tests/test_plan_footprint_cpu.py asserts that it does)
WITNESSED = ('tiny', 'tiny fp32', 'tiny fp32x', 'tiny keep', 'tiny keep_vox', 'tiny plms', 'tiny force_exchange', 'vq decode',
             'vq encode fp16', 'layout mc=128 crossattn', 'layout loop ddpm', 'layout loop ddpm keep', 'layout loop ddim keep eta')


LAYOUT_CONFIGS = tuple('layout mc=%d %s' % (mc, nm) for mc in (128, 384, 512) for nm in ('crossattn', 'no_t_emb', 'concat'))


def emit_layout(name):
    """(Builder, extended document) of the layout step tools/plan_dryrun.emit_layout_step_cpu emits, at the widths and flags of
    tests/golden/make_rows_routes.py"""
    import plan_dryrun
    mc = int(name.split('mc=')[1].split()[0])
    kw = {'crossattn': {}, 'no_t_emb': dict(enable_t_emb=False), 'concat': dict(concat=True)}[name.split()[-1]]
    log = []
    with recording_allocations(log):
        b, io = plan_dryrun.emit_layout_step_cpu(mc=mc, O=8, **kw)
    doc = extend(b, [io], None, log)
    bufs = mv.Buffers([b.keep, io], set(b.scratch))
    bufs.order, bufs.ordinal = list(doc['starts']), {s_: k for k, s_ in enumerate(doc['starts'])}
    doc['tensors'] = {k: [list(io[k].shape), bufs.ref(io[k].data_ptr(), k)] for k in ('x', 'objbuf', 'eps', 'step')}
    doc['values'] = dict(ucw=io['oe_w'])
    return b, doc


LOOP_CONFIGS = {'layout loop ddpm': {}, 'layout loop ddpm keep': dict(keep=True), 'layout loop ddim': dict(sampler='ddim', step_noise=False),
                'layout loop ddim keep eta': dict(sampler='ddim', keep=True, step_noise=True)}


def emit_layout_loop(name, mc=128, O=8, T=4, dev='cpu', fill=None, want_builder=False):
    """the extended document of the whole layout loop step (samplers.emit_layout_step WITH its update: es_ddpm_update,
    es_ddpm_update_keep or es_ddim_rows_update -- the kinds no other configuration here holds), on a CPU Builder.  The caller's inputs
    are x, the embedding columns of objbuf, the draws `noise` and, for the masked loops, x0 / mask / knoise (zero-filled when built)."""
    import torch
    from echoscene_amd import synth, config as escfg
    from echoscene_amd.model.unet import UNet1DModel
    from echoscene_amd.plan import Builder, GraphIndex, UNet1DWeights
    from echoscene_amd.samplers import _cap, _cpu_sd, emit_layout_step
    kw = dict(LOOP_CONFIGS[name])
    dev = torch.device(dev)
    mk = (lambda name, *shape: torch.zeros(*shape, device=dev)) if fill is None else fill
    net = UNet1DModel(**escfg.layout_denoiser_kwargs(mc))
    synth.seeded_fill_(net, prefix='dry.')
    w = UNet1DWeights(_cpu_sd(net), net, dev)
    _, triples = synth.synthetic_graph(O, seed=3)
    g = GraphIndex(triples, O, dev, capacity=_cap(triples.shape[0]))
    log = []
    with recording_allocations(log):
        b = Builder(dev)
        tables = dict(emb=None, emb_all=mk('emb_all', T, w.emb_all.N), t_lin=mk('t_lin', T, 64))
        coef, keep_tab = mk('coef', T, 5), mk('keep_tab', T, 2)
        io = emit_layout_step(b, w, g, mk('uc', O, 640), mk('temb', T, mc), tables, T, coef=coef, keep_tab=keep_tab, **kw)
    roots = [io, tables, coef, keep_tab]
    doc = extend(b, roots, None, log, n_steps=T)
    bufs = mv.Buffers([b.keep, roots], set(b.scratch))
    bufs.order, bufs.ordinal = list(doc['starts']), {s_: k for k, s_ in enumerate(doc['starts'])}
    # (the draws are `snoise` to step_inputs: per-step draws the caller fills; absent where no op reads them -- DDIM at eta = 0)
    doc['tensors'] = {'snoise' if k == 'noise' else k: [list(io[k].shape), bufs.ref(io[k].data_ptr(), k)]
                      for k in ('x', 'objbuf', 'step', 'noise') if io[k].untyped_storage().data_ptr() in bufs.ordinal}
    doc['values'] = dict(ucw=io['oe_w'])
    return (b, doc, io, roots) if want_builder else doc


# ------------------------------------------------------------------------------------------------ the analysis
class Ctx:
    def __init__(self, doc, kind, values):
        self.doc, self.kind, self.values, self.n_steps = doc, kind, values, doc.get('n_steps', 4)

    def ints(self, ptr, n):
        """the first n int32 values behind a pointer into an index tensor"""
        data = self.doc['ints'].get(ptr[0])
        if data is None:
            data = self.doc['ints'].get(str(ptr[0]))
        assert data is not None, 'the contents of index buffer %d are not part of the document' % ptr[0]
        i0 = ptr[1] // I32
        assert i0 + n <= len(data), 'index buffer %d holds %d values, %d are read' % (ptr[0], len(data), i0 + n)
        return data[i0:i0 + n]


_fields = {}


def op_fields(op):
    if not _fields:
        _fields.update(mv.field_names())
    member = mv.kind_members()[op[0]]
    return dict(zip(_fields[member], op[2:])) if member else {}


def op_footprint(doc, op):
    fn = footprint_table()[op[0]]
    if fn is None:
        return [], []
    return fn(op_fields(op), Ctx(doc, op[0], op[2:]))


def launch_groups(ops):
    """[(first op index, member count)] of the runtime's grouping, by tools/plan_dryrun.launches (the rule is not spelled again)"""
    import plan_dryrun
    from echoscene_amd import hip
    shim = SimpleNamespace(ops=[SimpleNamespace(kind=op[0], lane=op[1],
                                                u=SimpleNamespace(linear=SimpleNamespace(fuse_next=op_fields(op)['fuse_next'] if op[0] == hip.OP_LINEAR else 0)))
                                for op in ops])
    return [(i0, len(grp)) for i0, grp in plan_dryrun.launches(shim)]


class Order:
    """The partial order of one replay with es_plan_run's semantics: lane order; FORK(L) makes lane L wait for everything earlier on
    main; JOIN(L) makes main wait for lane L.  Vector clocks: clock[i][s] = the last op of stream s that op i is ordered behind.
    The members of one fused launch run as one grid: unordered among themselves."""

    def __init__(self, ops):
        from echoscene_amd import hip
        vc = {0: {}}
        self.clock, self.lane, self.group = [], [op[1] for op in ops], {}
        for i, op in enumerate(ops):
            kind, lane = op[0], op[1]
            if kind == hip.OP_FORK:
                vc.setdefault(lane, {})
                for s, k in vc[0].items():
                    vc[lane][s] = max(vc[lane].get(s, -1), k)
                self.clock.append(dict(vc[0]))
                self.lane[i] = 0
                continue
            if kind == hip.OP_JOIN:
                for s, k in vc.get(lane, {}).items():
                    vc[0][s] = max(vc[0].get(s, -1), k)
                self.clock.append(dict(vc[0]))
                self.lane[i] = 0
                continue
            vc.setdefault(lane, {})
            self.clock.append(dict(vc[lane]))
            vc[lane][lane] = i
        for i0, n in launch_groups(ops):
            for k in range(i0, i0 + n):
                self.group[k] = i0 if n > 1 else None

    def before(self, i, j):
        """op i happens before op j"""
        if i >= j:
            return False
        if self.group.get(i) is not None and self.group.get(i) == self.group.get(j):
            return False
        return self.clock[j].get(self.lane[i], -1) >= i

    def ordered(self, i, j):
        return self.before(i, j) if i < j else self.before(j, i)


class Cover:
    """a set of byte intervals"""

    def __init__(self):
        self.iv = []

    def add(self, spans):
        iv = sorted([lo, hi] for lo, hi in list(self.iv) + list(spans))
        out = []
        for lo, hi in iv:
            if out and lo <= out[-1][1]:
                out[-1][1] = max(out[-1][1], hi)
            else:
                out.append([lo, hi])
        self.iv = out

    def missing(self, spans):
        """bytes of ``spans`` not in the set: (count, first missing offset)"""
        import bisect
        los = [v[0] for v in self.iv]
        n, first = 0, None
        for lo, hi in spans:
            p = lo
            k = max(bisect.bisect_right(los, lo) - 1, 0)
            while p < hi:
                while k < len(self.iv) and self.iv[k][1] <= p:
                    k += 1
                if k < len(self.iv) and self.iv[k][0] <= p:
                    p = self.iv[k][1]
                    continue
                q = min(hi, self.iv[k][0]) if k < len(self.iv) else hi
                n += q - p
                first = p if first is None else first
                p = q
        return n, first


class Analysis:
    """footprints of an op list and every static check over them; ``findings``: messages that name configuration, op, kind and field"""

    def __init__(self, name, doc, ops=None):
        self.name, self.doc = name, doc
        self.ops = doc['ops'] if ops is None else ops
        self.fp = [op_footprint(doc, op) for op in self.ops]
        self.order = Order(self.ops)
        self.stats = dict(ops=len(self.ops), regions=sum(len(r) + len(w) for r, w in self.fp), pairs=0, scratch_bytes=0)

    def where(self, i, region=None):
        s = '%s: op %d (%s)' % (self.name, i, kind_name(self.ops[i][0]))
        return s if region is None else '%s field %s' % (s, region.field)

    def bounds(self):
        bad = []
        for i, (R, W) in enumerate(self.fp):
            for g in R + W:
                size = self.doc['buffers'][g.buf][0]
                if g.off < 0 or g.end > size:
                    bad.append('%s: ends %d bytes past buffer %d (%d bytes)' % (self.where(i, g), g.end - size, g.buf, size))
        return bad

    def self_aliasing(self):
        ok, bad = aliasing_ok(), []
        for i, (R, W) in enumerate(self.fp):
            allowed = ok.get(self.ops[i][0], {})
            for k, w in enumerate(W):
                for r in R:
                    if regions_overlap(w, r) and (w.field, r.field) not in allowed:
                        bad.append('%s: the write overlaps the read of field %s of the same op' % (self.where(i, w), r.field))
                for w2 in W[k + 1:]:
                    if regions_overlap(w, w2):
                        bad.append('%s: the write overlaps the write of field %s of the same op' % (self.where(i, w), w2.field))
        return bad

    def hazards(self):
        """two ops the order leaves unordered (two lanes, or two members of one launch): no write of one may overlap a read or a write
        of the other"""
        by_buf, bad = {}, []
        for i, (R, W) in enumerate(self.fp):
            for g in R:
                by_buf.setdefault(g.buf, []).append((i, g, False))
            for g in W:
                by_buf.setdefault(g.buf, []).append((i, g, True))
        examined = set()
        for buf, ent in by_buf.items():
            if not any(w for _, _, w in ent):
                continue
            for a in range(len(ent)):
                i, ga, wa = ent[a]
                for b in range(a + 1, len(ent)):
                    j, gb, wb = ent[b]
                    if i == j or not (wa or wb) or self.order.ordered(i, j):
                        continue
                    examined.add((i, j))
                    if regions_overlap(ga, gb):
                        same = self.order.group.get(i) is not None and self.order.group.get(i) == self.order.group.get(j)
                        (p, gp, wp), (q, gq, wq) = (ent[a], ent[b]) if wa else (ent[b], ent[a])
                        bad.append('%s %s what op %d (%s) field %s %s: %s' % (
                            self.where(q, gq), 'overwrites' if wq else 'reads', p, kind_name(self.ops[p][0]), gp.field, 'writes',
                            'members of one fused launch' if same else 'unordered (lanes %d and %d)' % (self.order.lane[p], self.order.lane[q])))
        self.stats['pairs'] = len(examined)          # unordered pairs that share a buffer one of them writes: regions compared
        n = len(self.ops)
        self.stats['unordered_pairs'] = sum(1 for i in range(n) for j in range(i + 1, n) if self.fp[i] != ([], []) and self.fp[j] != ([], [])
                                            and not self.order.ordered(i, j))
        return bad

    def _tracked(self):
        """buffer ordinal -> why a read of it must be preceded by a full write of the same replay"""
        t = {}
        for k, (_, _, scratch) in enumerate(self.doc['buffers']):
            if scratch:
                t[k] = 'scratch'
        for k in self.doc.get('empty', ()):
            t.setdefault(k, 'uninitialised (Builder.buf without zero)')
        return t

    def defined_before_read(self, inputs=(), tracked=None, failed=None):
        """In every linear extension of the order, a read of a byte of a scratch buffer -- or of a torch.empty buffer that is no
        declared input -- is preceded, in the same replay, by full writes covering it: only writes ordered BEFORE the reader count.
        ``tracked``: another {buffer: why} to hold to the rule; ``failed``: a set that receives the buffers that break it"""
        own = tracked is None
        tracked, bad = (self._tracked() if own else tracked), []
        writes = {}                                 # buffer -> [(op, spans)]; op -1: what the caller fills before the replay
        for g in inputs:                            # (a scratch buffer holds nothing of the caller's: a loaded model zero-fills it)
            if not self.doc['buffers'][g.buf][2]:
                writes.setdefault(g.buf, []).append((-1, g.spans()))
        proven = {}
        for j, (R, W) in enumerate(self.fp):
            reads = list(R) + [w for w in W if not w.full and not w.internal]
            for g in reads:
                if g.buf not in tracked:
                    continue
                cov = Cover()
                for i, spans in writes.get(g.buf, ()):
                    if i < 0 or self.order.before(i, j):
                        cov.add(spans)
                n, first = cov.missing(g.spans())
                if n:
                    bad.append('%s: reads %d bytes of %s buffer %d (first at +%d) that no earlier op of the replay has fully written' % (
                        self.where(j, g), n, tracked[g.buf], g.buf, first))
                    if failed is not None:
                        failed.add(g.buf)
                else:
                    proven.setdefault(g.buf, Cover()).add(g.spans())
            for g in W:
                if g.full and not g.internal and g.buf in tracked:
                    writes.setdefault(g.buf, []).append((j, g.spans()))
        if own:
            self.stats['scratch_bytes'] = sum(hi - lo for k, c in proven.items() if tracked[k] == 'scratch' for lo, hi in c.iv)
        return bad

    def could_be_scratch(self, keep=(), inputs=()):
        """non-scratch fp32 / f16 buffers the plan writes that would qualify: every read is covered by earlier full writes of the replay
        and the caller does not take them back (``keep``: ordinals of result tensors)"""
        written = {g.buf for _, W in self.fp for g in W if not g.internal}
        cand = {k: 'candidate' for k, (size, dtypes, scratch) in enumerate(self.doc['buffers'])
                if not scratch and k not in keep and k in written and set(dtypes) <= {'float32', 'float16'}}
        failed = set()
        self.defined_before_read(inputs, tracked=cand, failed=failed)
        return sorted(set(cand) - failed)

    def all_findings(self, inputs=()):
        return self.bounds() + self.self_aliasing() + self.hazards() + self.defined_before_read(inputs)
