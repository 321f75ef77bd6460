"""GPU tests of box-preserving sampling: the layout update that carries the kept rows (es_ddpm_update_keep) alone through the C ABI,
the masked ancestral loop against a golden made around the reference's own p_sample_sg / q_sample
(tests/golden/make_golden_keep_boxes.py) and, bit for bit, against the composition of the existing pieces, the fused layout + shape
graph, the scene calls, the model file, and es_box_prescale.  Bars: the layout loop's own (_close(..., 2e-4) of
test_layout_loop_tiny_100_steps_vs_reference_golden: same network, length and arithmetic), the scene calls' 1e-4 of
test_sgdiff_keep_shapes_vs_composed_reference_golden, the box helpers' atol = rtol = 1e-6; everything else is torch.equal."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import load_golden
from echoscene_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda')


def _rnd(shape, seed, scale=1.0):
    return torch.from_numpy((np.random.RandomState(seed).standard_normal(shape) * scale).astype(np.float32))


# ------------------------------------------------------------------------------------------------ the kernel alone
N_TAB = 20


def _ref_update(x, eps, nz, c, clip, mask, x0, tab, kn, st):
    """the kernel's expressions in fp32 torch on the CPU: one torch op per product and per sum, so nothing is contracted"""
    e = eps[0]
    for j in range(1, eps.shape[0]):
        e = e + eps[j]
    t1 = c[0] * x
    t2 = c[1] * e
    p0 = t1 - t2
    if clip:
        p0 = torch.clamp(p0, -1.0, 1.0)
    m1 = c[2] * p0
    m2 = c[3] * x
    mean = m1 + m2
    sn = c[4] * nz
    gen = mean + sn
    if st + 1 < N_TAB:
        kp = tab[st + 1, 0] * x0
        kq = tab[st + 1, 1] * kn[st + 1]
        kept = kp + kq
    else:
        kept = x0.clone()
    return torch.where(mask[:, None].bool(), kept, gen)


@pytest.mark.parametrize('O', [1, 3, 512, 513])
def test_ddpm_update_keep_kernel_vs_torch_bitwise(dev, O):
    """es_ddpm_update_keep through the C ABI at n = 8, 24, 4096 (the last size of the one-workgroup path) and 4104 (the first of the
    multi-workgroup path): masks none / all / first-and-last kept, steps 0 / middle / n_tab - 1 (with one NaN row behind tab and
    keep_noise, which must not be read), eps as 1 and 2 slabs, clip_x0 0 / 1, inc_step 0 / 1 with the counter checked.  A fourth
    mask case, 'plain', is es_ddpm_update with UpdateArgs -- no x0 / tab / keep_noise at all -- against the reference with a zero
    mask: it runs the same kernel with mask == NULL."""
    from echoscene_amd import hip
    from echoscene_amd.schedules import LayoutSchedule
    L = hip.lib()
    sched = LayoutSchedule(N_TAB)
    row, n = 8, O * 8
    x_in = _rnd((O, row), 1, 1.5)
    eps = _rnd((2, O, row), 2)
    noise = _rnd((N_TAB, O, row), 3)
    x0 = _rnd((O, row), 4, 0.6)
    kn = torch.cat([_rnd((N_TAB, O, row), 5), torch.full((1, O, row), float('nan'))])
    tab = torch.cat([sched.keep_tab, torch.full((1, 2), float('nan'))])
    coef = sched.coef
    masks = {'none': torch.zeros(O), 'all': torch.ones(O), 'mixed': torch.zeros(O)}
    masks['mixed'][0] = masks['mixed'][-1] = 1.0
    if O > 3:
        masks['mixed'][torch.from_numpy(np.random.RandomState(6).permutation(O)[:O // 3])] = 1.0
    d = lambda t: t.contiguous().to(dev)
    x_d, eps_d, nz_d, x0_d, kn_d, tab_d, coef_d = d(x_in), d(eps), d(noise), d(x0), d(kn), d(tab), d(coef)
    step_d = torch.zeros(1, dtype=torch.int32, device=dev)
    a = hip.DdpmKeepArgs()
    a.x, a.eps, a.noise, a.coef, a.step = x_d.data_ptr(), eps_d.data_ptr(), nz_d.data_ptr(), coef_d.data_ptr(), step_d.data_ptr()
    a.eps_slab_stride, a.noise_stride, a.coef_stride, a.n = n, n, 5, n
    a.x0, a.keep_noise, a.tab = x0_d.data_ptr(), kn_d.data_ptr(), tab_d.data_ptr()
    a.keep_noise_stride, a.n_tab, a.row = n, N_TAB, row
    u = hip.UpdateArgs()
    u.x, u.eps, u.noise, u.coef, u.step = a.x, a.eps, a.noise, a.coef, a.step
    u.eps_slab_stride, u.noise_stride, u.coef_stride, u.n = n, n, 5, n
    masks['plain'] = torch.zeros(O)
    checked = 0
    for mname, mask in masks.items():
        mask_d = d(mask)
        a.mask = mask_d.data_ptr()
        plain = mname == 'plain'
        for st in (0, 7, N_TAB - 1):
            for nslab in (1, 2):
                for clip in (0, 1):
                    for inc in (0, 1):
                        x_d.copy_(x_in)
                        step_d.fill_(st)
                        a.eps_nslab, a.clip_x0, a.inc_step = nslab, clip, inc
                        u.eps_nslab, u.clip_x0, u.inc_step = nslab, clip, inc
                        if plain:
                            hip.check(L.es_ddpm_update(C.byref(u), hip.current_stream()), 'es_ddpm_update')
                        else:
                            hip.check(L.es_ddpm_update_keep(C.byref(a), hip.current_stream()), 'es_ddpm_update_keep')
                        got, stc = x_d.cpu(), int(step_d.item())
                        ref = _ref_update(x_in, eps[:nslab], noise[st], coef[st], clip, mask, x0, tab, kn, st)
                        tag = 'O=%d mask=%s step=%d slabs=%d clip=%d inc=%d' % (O, mname, st, nslab, clip, inc)
                        assert torch.isfinite(got).all(), tag
                        assert torch.equal(got, ref), tag + ': max abs diff %.3e' % (got - ref).abs().max().item()
                        assert stc == st + inc, tag + ': step counter %d' % stc
                        if st == N_TAB - 1:
                            assert torch.equal(got[mask.bool()], x0[mask.bool()]), tag
                        checked += 1
    assert checked == 96
    # the two halves really differ on these inputs (a kernel that ignored the mask would not pass)
    r0 = _ref_update(x_in, eps[:1], noise[0], coef[0], 0, masks['none'], x0, tab, kn, 0)
    r1 = _ref_update(x_in, eps[:1], noise[0], coef[0], 0, masks['all'], x0, tab, kn, 0)
    assert not torch.equal(r0, r1)


# ------------------------------------------------------------------------------------------------ the tiny loop
@pytest.fixture(scope='module')
def tiny(dev):
    """one LayoutDenoiser (tiny width, O = 8, T = 100: the model of layout_loop_tiny) and the inputs of layout_keep_tiny, shared by
    the loop tests; the unmasked result is computed once"""
    from test_hip_rows import _layout
    g, gp = load_golden('layout_keep_tiny'), load_golden('layout_loop_tiny')
    den = _layout(dev, 128, 128, 'unet1d_tiny.', 100)
    xs, qs = [int(v) for v in g['seeds']]
    keep = g['keep'].long()
    x0 = torch.zeros(8, 8)
    x0[keep] = _rnd((len(keep), 8), xs, 0.5)
    assert torch.equal(x0, g['x0'])
    table = torch.stack([_rnd((8, 8), qs + k) for k in range(100)])
    mask = torch.zeros(8)
    mask[keep] = 1.0
    noise = synth.layout_noise(8, 8, 100, seed=7)
    plain = den.sample(gp['obj_embed'], gp['triples'], noise)
    return dict(g=g, gp=gp, den=den, keep=keep, gen=(mask == 0).nonzero().flatten(), x0=x0, table=table, mask=mask, noise=noise,
                oe=gp['obj_embed'], triples=gp['triples'], plain=plain)


@pytest.mark.parametrize('use_graph', [False, True])
def test_layout_keep_tiny_vs_reference_golden(dev, tiny, use_graph):
    """LayoutDenoiser.sample(x0, mask, keep_noise) against layout_keep_tiny: generated rows inside the loop test's own bar, kept rows
    x0 bit for bit; a second call and a call after poison_scratch() give the same bits; the kept nodes are context (the masked
    golden's generated rows differ from the unmasked golden's by more than ten times the bar, and so do this run's)."""
    from test_hip_rows import _close
    t = tiny
    den, g, gen, keep = t['den'], t['g'], t['gen'], t['keep']
    kw = dict(x0=t['x0'], mask=t['mask'], keep_noise=t['table'], use_graph=use_graph)
    x = den.sample(t['oe'], t['triples'], t['noise'], **kw)
    d = (x.cpu()[gen] - g['x_final'][gen]).abs().max().item()
    print('layout keep tiny (100 steps, nodes %s kept, graph=%s): generated rows vs golden: max abs err %.3e' % (keep.tolist(), use_graph, d))
    _close(x[gen], g['x_final'][gen], 2e-4)
    assert torch.equal(x.cpu()[keep], t['x0'][keep]), 'kept rows are x0, bit for bit'
    assert torch.equal(den.sample(t['oe'], t['triples'], t['noise'], **kw), x)
    den._last['plan'].poison_scratch()
    assert torch.equal(den.sample(t['oe'], t['triples'], t['noise'], **kw), x)
    bar = 2e-4 + 1e-5 * t['gp']['x_final'].abs().max().item()
    ctx_g = (g['x_final'][gen] - t['gp']['x_final'][gen]).abs().amax(dim=1)
    ctx_x = (x.cpu()[gen] - t['plain'].cpu()[gen]).abs().amax(dim=1)
    print('context: per generated row max |masked - unmasked|: golden %s, this run %s' % (
        ['%.2e' % v for v in ctx_g.tolist()], ['%.2e' % v for v in ctx_x.tolist()]))
    assert float(ctx_g.min()) > 10 * bar and float(ctx_x.min()) > 10 * bar


@pytest.mark.parametrize('use_graph', [False, True])
def test_layout_keep_equals_blend_before_every_step_bitwise(dev, tiny, use_graph):
    """the fused form == the definition, bit for bit on every row: the UNMASKED plan replayed one iteration at a time with the blend
    done between iterations in torch (one op per product and per sum), x0 written after the last one; also the state in front of
    the first and of the last denoiser call is q_sample of the kept rows bit for bit, and the golden's to the ulp of a table entry
    (priming, and what a run stopped early leaves)."""
    t = tiny
    den, keep, g = t['den'], t['keep'], t['g']
    x = den.sample(t['oe'], t['triples'], t['noise'], x0=t['x0'], mask=t['mask'], keep_noise=t['table'], use_graph=use_graph)
    st = den._plan_for(t['oe'], t['triples'])
    assert st['x0'] is None                                    # the unmasked cache entry
    st['noise'][:101].copy_(t['noise'].to(dev))
    st['x'].copy_(st['noise'][0])
    x0d, knd, tab, kd = t['x0'].to(dev), t['table'].to(dev), den.keep_tab, keep.to(dev)
    for i in range(100):
        p = tab[i, 0] * x0d
        q = tab[i, 1] * knd[i]
        st['x'][kd] = (p + q)[kd]
        st['plan'].sample(st['step'], i, 1, use_graph=use_graph)
    st['x'][kd] = x0d[kd]
    assert torch.equal(st['x'], x), 'max abs diff %.3e' % (st['x'] - x).abs().max().item()
    # priming: x_T with the kept rows at q_sample(x0, T-1, keep_noise[0]) -- the reference's bits
    sk = den._plan_for(t['oe'], t['triples'], keep=True)
    den._fill_keep(sk, t['x0'], t['mask'], t['table'])
    sk['noise'][:101].copy_(t['noise'].to(dev))
    sk['x'].copy_(sk['noise'][0])
    den._prime_keep(sk)
    # (the factors come from the table of THIS process: the reference forms them with torch.sqrt on fp32, whose last bit differs
    #  between hosts -- 1.2e-7 on the kept rows against the golden's host was seen -- so the bitwise statement is against q_sample
    #  restated with den.keep_tab, and the golden is met to the ulp of a table entry: 2^-24 relative per factor, two products and a
    #  sum of values below 4 -> atol = rtol = 1e-6)
    tab_c = den.keep_tab.cpu()

    def q_sample(i):
        p = tab_c[i, 0] * t['x0']
        q = tab_c[i, 1] * t['table'][i]
        return p + q
    want = t['noise'][0].clone()
    want[keep] = q_sample(0)[keep]
    d0 = (sk['x'].cpu() - g['seen_first']).abs()
    print('primed x_T vs the golden: max abs diff per row %s' % ['%.3e' % v for v in d0.amax(dim=1).tolist()])
    assert torch.equal(sk['x'].cpu(), want)
    assert torch.equal(sk['x'].cpu()[t['gen']], g['seen_first'][t['gen']])
    assert torch.allclose(sk['x'].cpu(), g['seen_first'], atol=1e-6, rtol=1e-6)
    # stopped one iteration early: the kept rows hold the LAST iteration's forward-noised value (documented), not x0
    x99 = den.sample(t['oe'], t['triples'], t['noise'], n_steps=99, x0=t['x0'], mask=t['mask'], keep_noise=t['table'], use_graph=use_graph)
    assert torch.equal(x99.cpu()[keep], q_sample(99)[keep]) and not torch.equal(x99.cpu()[keep], t['x0'][keep])
    assert torch.allclose(x99.cpu()[keep], g['seen_last'][keep], atol=1e-6, rtol=1e-6)


def test_layout_keep_edge_masks_and_clip(dev, tiny):
    """all-zero mask == the unmasked sample with the same noise, bit for bit; all-one mask -> x0; clip_denoised=True combines with
    keep (another cache entry) and meets the golden's clip variant, kept rows unclipped; argument errors."""
    from test_hip_rows import _close
    t = tiny
    den, g, gen, keep = t['den'], t['g'], t['gen'], t['keep']
    a = (t['oe'], t['triples'], t['noise'])
    big = _rnd((8, 8), 9, 2.0)                                  # values outside [-1, 1]: a kept row is never clipped
    x = den.sample(*a, x0=big, mask=torch.zeros(8), keep_noise=t['table'])
    assert torch.equal(x, t['plain']), 'an all-zero mask: nothing is kept'
    x = den.sample(*a, x0=big, mask=torch.ones(8), keep_noise=t['table'], clip_denoised=True)
    assert torch.equal(x.cpu(), big)
    xc = den.sample(*a, x0=t['x0'], mask=t['mask'], keep_noise=t['table'], clip_denoised=True)
    _close(xc[gen], g['x_final_clip'][gen], 2e-4)
    assert torch.equal(xc.cpu()[keep], t['x0'][keep])
    assert len([k for k in den._plans if 'keep' in k]) == 2 and any('clip' in k and 'keep' in k for k in den._plans)
    # mask=None afterwards: the old loop
    assert torch.equal(den.sample(*a), t['plain'])
    with pytest.raises(ValueError):
        den.sample(*a, x0=t['x0'])
    with pytest.raises(ValueError):
        den.sample(*a, keep_noise=t['table'])
    with pytest.raises(ValueError):
        den.sample(*a, x0=t['x0'], mask=torch.tensor([0.5, 0, 1, 1, 0, 0, 0, 0]))
    with pytest.raises(ValueError):
        den.sample(*a, x0=t['x0'][:, :6], mask=t['mask'])
    with pytest.raises(ValueError):
        den.sample(*a, x0=t['x0'], mask=t['mask'], keep_noise=t['table'][:50])
    # drawn on the device when None: kept rows still x0
    assert torch.equal(den.sample(*a, x0=t['x0'], mask=t['mask']).cpu()[keep], t['x0'][keep])


def test_layout_keep_plan_on_the_device(dev, tiny):
    """the plans the denoiser really runs: keep == the unmasked plan with only the last op replaced, and the same number of launches
    (the unmasked list against the parent commit's is tests/test_keep_boxes_cpu.py's, at the default context width)"""
    from echoscene_amd import hip
    from test_hip_keep import op_signature
    t = tiny
    den = t['den']
    plain = den._plan_for(t['oe'], t['triples'])['plan']
    keep = den._plan_for(t['oe'], t['triples'], keep=True)['plan']
    sp, sk = op_signature(plain), op_signature(keep)
    assert len(sp) == len(sk) and sk[:-1] == sp[:-1] and sp[-1][0] == hip.OP_DDPM and sk[-1][0] == hip.OP_DDPM_KEEP
    assert all(s_[0] != hip.OP_DDPM_KEEP for s_ in sp)
    assert plain.n_launches == keep.n_launches and plain.n_ops == keep.n_ops


# ------------------------------------------------------------------------------------------------ the fused graph
def test_fused_graph_with_kept_boxes(dev, tiny):
    """sample_layout_and_shape with the keep plan as the side branch (25 layout steps per DDIM step of a 4-step tiny shape denoiser):
    boxes == LayoutDenoiser.sample alone on the same inputs, latents == the call without box keeping, both bit for bit."""
    from echoscene_amd.samplers import sample_layout_and_shape
    from test_hip_keep import _shape
    t = tiny
    lay, shp = t['den'], _shape(dev)
    uc, n1 = _rnd((8, 1, 64), 52), synth.shape_noise(seed=7)
    alone = lay.sample(t['oe'], t['triples'], t['noise'], x0=t['x0'], mask=t['mask'], keep_noise=t['table'])
    x, z = sample_layout_and_shape(lay, shp, t['oe'], t['triples'], uc, layout_noise=t['noise'], shape_noise=n1,
                                   box_x0=t['x0'], box_mask=t['mask'], box_keep_noise=t['table'])
    assert torch.equal(x, alone), 'max abs diff %.3e' % (x - alone).abs().max().item()
    x_p, z_p = sample_layout_and_shape(lay, shp, t['oe'], t['triples'], uc, layout_noise=t['noise'], shape_noise=n1)
    assert torch.equal(z, z_p) and torch.equal(x_p, t['plain'])
    with pytest.raises(ValueError):
        sample_layout_and_shape(lay, shp, t['oe'], t['triples'], uc, layout_noise=t['noise'], shape_noise=n1, box_x0=t['x0'])


# ------------------------------------------------------------------------------------------------ the public interface
def test_sgdiff_keep_boxes_vs_composed_reference_golden():
    """'echolayout' sample_box_and_shape and 'echoscene' sample_boxes_and_shape_with_changes with keep_box_nodes / keep_boxes against
    scene_keep_boxes_tiny (the reference's scene calls with its layout loop replaced by the masked loop composed of its own p_sample_sg
    / q_sample); bars of test_sgdiff_keep_shapes_vs_composed_reference_golden (boxes 1e-4 of the tensor scale).  Kept rows are the
    caller's numbers bit for bit; a result fed back as keep_boxes comes back unchanged; the new argument errors."""
    from test_hip_keep import _build_sgdiff, _rel
    g = load_golden('scene_keep_boxes_tiny')
    objs, triples = g['objs'], g['triples']
    O = objs.shape[0]
    tf, rf = synth.synthetic_features(O, triples.shape[0], seed=9)
    keep = [int(v) for v in g['keep']]
    xs, qs = [int(v) for v in g['seeds']]
    boxes = _rnd((len(keep), 8), xs, 0.5)
    table = torch.stack([_rnd((O, 8), qs + k) for k in range(100)])
    a = (objs.cuda(), triples.cuda(), tf.cuda(), rf.cuda())
    cat = lambda d: torch.cat([d['sizes'], d['translations'], d['angles']], 1)
    ln = synth.layout_noise(O, 8, 100, seed=7)
    ml = _build_sgdiff('echolayout')
    d = ml.sample_box_and_shape(*a, layout_noise=ln, keep_box_nodes=keep, keep_boxes=boxes, keep_box_noise=table)
    for k in ('sizes', 'translations', 'angles'):
        e = _rel(d[k], g['lay_' + k])
        print('scene keep boxes, echolayout %s: rel err %.2e' % (k, e))
        assert e < 1e-4, k
    assert torch.equal(cat(d).cpu()[keep], boxes), 'kept rows are the caller\'s boxes, bit for bit'
    # duplicates / out-of-range entries: the keep_selection convention
    d2 = ml.sample_box_and_shape(*a, layout_noise=ln, keep_box_nodes=keep + [keep[0], 99], keep_box_noise=table,
                                 keep_boxes=torch.cat([boxes, boxes[:2] * 0]))
    assert torch.equal(cat(d2), cat(d))
    # a result fed straight back: every node kept -> the same rows
    d3 = ml.sample_box_and_shape(*a, layout_noise=ln, keep_box_nodes=list(range(O)), keep_boxes=cat(d))
    assert torch.equal(cat(d3), cat(d))
    np.random.seed(5)
    k4, d4 = ml.sample_boxes_and_shape_with_changes(*a, *a, [1], layout_noise=ln, keep_box_nodes=keep, keep_boxes=boxes, keep_box_noise=table)
    assert torch.equal(cat(d4).cpu()[keep], boxes)
    d5 = ml.sample_boxes_and_shape_with_additions(*a, *a, [], layout_noise=ln, keep_box_nodes=keep, keep_boxes=boxes, keep_box_noise=table)
    assert torch.equal(cat(d5).cpu()[keep], boxes)
    with pytest.raises(ValueError):
        ml.sample_box_and_shape(*a, layout_noise=ln, keep_box_nodes=keep)
    with pytest.raises(ValueError):
        ml.sample_box_and_shape(*a, layout_noise=ln, keep_boxes=boxes)
    with pytest.raises(ValueError):
        ml.sample_box_and_shape(*a, layout_noise=ln, keep_box_nodes=keep, keep_boxes=boxes[:, :6])
    with pytest.raises(ValueError):                                                      # _no_keep_without_shapes still fires
        ml.sample_box_and_shape(*a, keep_nodes=keep, keep_sdfs=torch.zeros(len(keep), 1, 64, 64, 64), layout_noise=ln)
    # 'echoscene', an editing call, shapes generated too (the fused graph with the keep plan as its side branch)
    m = _build_sgdiff('echoscene')
    np.random.seed(5)
    k6, d6 = m.sample_boxes_and_shape_with_changes(*a, *a, [1], gen_shape=True, layout_noise=ln, shape_noise=synth.shape_noise(seed=7),
                                                   keep_box_nodes=keep, keep_boxes=boxes, keep_box_noise=table)
    for k in ('sizes', 'translations', 'angles'):
        e = _rel(d6[k], g['sc_chg_' + k])
        print('scene keep boxes, echoscene with_changes %s: rel err %.2e' % (k, e))
        assert e < 1e-4, k
    assert torch.equal(cat(d6).cpu()[keep], boxes) and k6.flatten().tolist() == g['sc_chg_keep'].flatten().tolist() == [1, 0] + [1] * (O - 2)
    assert tuple(d6['shapes'].shape) == (O, 1, 64, 64, 64)
    # gen_shape off: the same boxes through the plain layout call; both keyword families at once
    np.random.seed(5)
    k7, d7 = m.sample_boxes_and_shape_with_changes(*a, *a, [1], gen_shape=False, layout_noise=ln, keep_box_nodes=keep, keep_boxes=boxes,
                                                   keep_box_noise=table)
    assert torch.equal(cat(d7), cat(d6))
    sdfs = synth.ellipsoid_sdfs(2, seed=83)
    d8 = m.sample_box_and_shape(*a, gen_shape=True, layout_noise=ln, shape_noise=synth.shape_noise(seed=7), keep_nodes=[0, 2], keep_sdfs=sdfs,
                                keep_box_nodes=keep, keep_boxes=boxes, keep_box_noise=table)
    assert torch.equal(cat(d8).cpu()[keep], boxes) and torch.equal(d8['shapes'][[0, 2]].cpu(), sdfs)
    with pytest.raises(ValueError):                                                      # existing error, untouched
        m.sample_box_and_shape(*a, gen_shape=False, keep_nodes=[0], keep_sdfs=sdfs[:1], layout_noise=ln)


# ------------------------------------------------------------------------------------------------ the model file
def test_layout_keep_model_file(dev, tiny, tmp_path):
    """save_model(keep=True) -> es_model_load -> es_layout_sample_keep through ctypes == LayoutDenoiser.sample, bit for bit; a request
    to run past the table is refused with an error."""
    from echoscene_amd import hip
    t = tiny
    den = t['den']
    L = hip.lib()
    ref = den.sample(t['oe'], t['triples'], t['noise'], x0=t['x0'], mask=t['mask'], keep_noise=t['table'])
    path = str(tmp_path / 'layout_keep.esm')
    den.save_model(path, t['oe'], t['triples'], keep=True)
    m = L.es_model_load(path.encode())
    assert m, L.es_last_error()
    try:
        for name, nbytes in ((b'x0', 256), (b'mask', 32), (b'knoise', 100 * 256), (b'ktab', 800)):
            ptr, nb = C.c_void_p(), C.c_size_t()
            hip.check(L.es_model_region(C.c_void_p(m), name, C.byref(ptr), C.byref(nb)), 'es_model_region')
            assert nb.value == nbytes, name
        nz, x0, mk, kn = (v.contiguous().to(dev) for v in (t['noise'], t['x0'], t['mask'], t['table']))
        out = torch.full((8, 8), float('nan'), device=dev)
        p = lambda v: C.c_void_p(v.data_ptr())
        hip.check(L.es_layout_sample_keep(C.c_void_p(m), p(nz), 101, 100, p(x0), p(mk), p(kn), p(out), hip.current_stream()),
                  'es_layout_sample_keep')
        torch.cuda.synchronize()
        assert torch.equal(out, ref), 'max abs diff %.3e' % (out - ref).abs().max().item()
        nz2 = torch.zeros(102, 8, 8, device=dev)
        rc = L.es_layout_sample_keep(C.c_void_p(m), p(nz2), 102, 101, p(x0), p(mk), p(kn), p(out), hip.current_stream())
        assert rc != 0 and b'schedule' in L.es_last_error()
        assert L.es_model_run(C.c_void_p(m), 50, 51, hip.current_stream()) != 0 and b'schedule' in L.es_last_error()
    finally:
        L.es_model_free(C.c_void_p(m))
    # a model saved without keep has no masked update: refused, not run
    path2 = str(tmp_path / 'layout_plain.esm')
    den.save_model(path2, t['oe'], t['triples'])
    m2 = L.es_model_load(path2.encode())
    assert m2, L.es_last_error()
    try:
        assert L.es_layout_sample_keep(C.c_void_p(m2), p(nz), 101, 100, p(x0), p(mk), p(kn), p(out), hip.current_stream()) != 0
    finally:
        L.es_model_free(C.c_void_p(m2))


# ------------------------------------------------------------------------------------------------ the box helpers
def test_box_prescale_vs_reference_golden():
    """es_box_prescale against box_pre (the reference's scale_box_params, 6 and 7 columns, with the statistics of the box_post fixture,
    and preprocess_angle2sincos) at the box_post test's own bar, atol = rtol = 1e-6; descale(scale(x)) returns x inside the same bar."""
    from echoscene_amd.postprocess import scale_box_params, preprocess_angle2sincos, descale_box_params, postprocess_sincos2arctan
    g = load_golden('box_pre')
    stats = g['stats'].double().numpy()
    assert np.array_equal(stats, load_golden('box_post')['stats'].double().numpy())
    b6 = g['boxes'].cuda()
    r = scale_box_params(b6, stats=stats)
    assert r.data_ptr() == b6.data_ptr()
    assert torch.allclose(b6.cpu(), g['boxes_out'], atol=1e-6, rtol=1e-6), (b6.cpu() - g['boxes_out']).abs().max()
    b7 = g['boxes7'].cuda()
    scale_box_params(b7, stats=stats, angle=True)
    assert torch.allclose(b7.cpu(), g['boxes7_out'], atol=1e-6, rtol=1e-6), (b7.cpu() - g['boxes7_out']).abs().max()
    wide = torch.full((33, 9), 7.0).cuda()                      # a wider matrix: only the first ncol columns are touched
    wide[:, :6] = g['boxes'].cuda()
    scale_box_params(wide, stats=stats)
    assert torch.equal(wide[:, :6], b6) and bool((wide[:, 6:] == 7.0).all())
    sc = preprocess_angle2sincos(g['angle'].cuda())
    assert tuple(sc.shape) == (33, 2)
    assert torch.allclose(sc.cpu(), g['sincos'], atol=1e-6, rtol=1e-6)
    # round trips
    descale_box_params(b6, stats=stats)
    assert torch.allclose(b6.cpu(), g['boxes'], atol=1e-6, rtol=1e-6), (b6.cpu() - g['boxes']).abs().max()
    descale_box_params(b7, stats=stats, angle=True)
    assert torch.allclose(b7.cpu(), g['boxes7'], atol=1e-6, rtol=1e-6), (b7.cpu() - g['boxes7']).abs().max()
    assert torch.allclose(postprocess_sincos2arctan(sc).cpu(), g['angle'], atol=1e-6, rtol=1e-6)
    with pytest.raises(ValueError):
        scale_box_params(g['boxes'], stats=stats)              # a CPU tensor
    with pytest.raises(NotImplementedError):
        scale_box_params(g['boxes'].cuda(), stats=stats[:12])
