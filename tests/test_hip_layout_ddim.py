"""GPU tests of strided DDIM sampling of the layout loop: the update kernel (es_ddim_rows_update) alone through the C ABI, bit for bit
against an fp32 restatement and against es_ddim_update; the loops against goldens made with the reference's own DDIMSampler on the
layout denoiser (tests/golden/make_golden_layout_ddim.py) at the rows path's bar, atol 1e-4 + rtol 1e-4 (the fp32
restatement of tests/test_layout_ddim_cpu.py meets every golden at that bar, the S = 100 case included, so no case has another bar);
the masked loop; the bit-for-bit identities (graph / eager, repeatability, the default loop untouched, the fused graph, the draw
order); the model file; and the scene calls."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import load_golden
from echoscene_amd import synth, config as escfg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda')


def _rnd(shape, seed, scale=1.0):
    return torch.from_numpy((np.random.RandomState(seed).standard_normal(shape) * scale).astype(np.float32))


def _bar(got, ref, what):
    """atol 1e-4 + rtol 1e-4, every figure printed before it is asserted"""
    got, ref = got.detach().cpu().float(), ref.detach().cpu().float()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = (got - ref).abs()
    print('%s: max abs err %.3e (ref scale %.3e), worst err / bar %.3f' % (
        what, err.max().item(), ref.abs().max().item(), (err / (1e-4 + 1e-4 * ref.abs())).max().item()))
    assert torch.isfinite(got).all(), what
    assert torch.allclose(got, ref, atol=1e-4, rtol=1e-4), what


# ------------------------------------------------------------------------------------------------ 1: the kernel alone
N_TAB = 20


def _ref_rows(x, eps, nz, c, mask, x0, tab, kn, st):
    """the kernel's expressions in fp32 torch on the CPU: one torch op per product, sum and quotient, so nothing is contracted"""
    e = eps[0]
    for j in range(1, eps.shape[0]):
        e = e + eps[j]
    t1 = c[0] * e
    d = x - t1
    px0 = d / c[1]
    m1 = c[2] * px0
    m2 = c[3] * e
    gen = m1 + m2
    if nz is not None:
        sn = c[4] * nz
        gen = gen + sn
    if mask is None:
        return gen
    if st + 1 < N_TAB:
        kp = tab[st + 1, 0] * x0
        kq = tab[st + 1, 1] * kn[st + 1]
        kept = kp + kq
    else:
        kept = x0.clone()
    return torch.where(mask[:, None].bool(), kept, gen)


@pytest.mark.parametrize('O', [4, 520])
def test_ddim_rows_update_kernel_vs_torch_bitwise(dev, O):
    """es_ddim_rows_update through the C ABI at n = 32 (one workgroup, which advances the counter itself) and n = 4160 (just past the
    4096 switch: 17 workgroups and the separate increment): eps as 1 and 2 slabs, with and without noise, without a mask / all-zero /
    mixed, the counter at 0, in the middle and at the last row (one NaN row behind tab and keep_noise must not be read; kept rows are
    then x0's bits), x and the step counter compared bit for bit; mask-0 rows torch.equal to es_ddim_update on the same inputs."""
    from echoscene_amd import hip
    from echoscene_amd.schedules import LayoutSchedule, LayoutDdimSchedule
    L = hip.lib()
    base = LayoutSchedule(1000)
    sched = LayoutDdimSchedule(base, N_TAB, 0.7)
    assert tuple(sched.coef.shape) == (N_TAB, 5)
    row, n = 8, O * 8
    x_in = _rnd((O, row), 1, 1.5)
    eps = _rnd((2, O, row), 2)
    noise = _rnd((N_TAB, O, row), 3)
    x0 = _rnd((O, row), 4, 0.6)
    kn = torch.cat([_rnd((N_TAB, O, row), 5), torch.full((1, O, row), float('nan'))])
    tab = torch.cat([sched.keep_tab, torch.full((1, 2), float('nan'))])
    coef = sched.coef
    masks = {'nomask': None, 'zeros': torch.zeros(O), 'mixed': torch.zeros(O)}
    masks['mixed'][0] = masks['mixed'][-1] = 1.0
    if O > 4:
        masks['mixed'][torch.from_numpy(np.random.RandomState(6).permutation(O)[:O // 3])] = 1.0
    d = lambda t: t.contiguous().to(dev)
    x_d, eps_d, nz_d, x0_d, kn_d, tab_d, coef_d = d(x_in), d(eps), d(noise), d(x0), d(kn), d(tab), d(coef)
    step_d = torch.zeros(1, dtype=torch.int32, device=dev)
    x2_d = torch.empty_like(x_d)
    checked = 0
    for mname, mask in masks.items():
        mask_d = None if mask is None else d(mask)
        for st in (0, 7, N_TAB - 1):
            for nslab in (1, 2):
                for with_noise in (False, True):
                    for inc in (0, 1):
                        a = hip.DdpmKeepArgs()
                        a.x, a.eps, a.coef, a.step = x_d.data_ptr(), eps_d.data_ptr(), coef_d.data_ptr(), step_d.data_ptr()
                        a.eps_nslab, a.eps_slab_stride, a.coef_stride, a.n, a.n_tab, a.row, a.inc_step = nslab, n, 5, n, N_TAB, row, inc
                        if with_noise:
                            a.noise, a.noise_stride = nz_d.data_ptr(), n
                        if mask is not None:
                            a.x0, a.mask, a.keep_noise, a.tab = x0_d.data_ptr(), mask_d.data_ptr(), kn_d.data_ptr(), tab_d.data_ptr()
                            a.keep_noise_stride = n
                        x_d.copy_(x_in)
                        step_d.fill_(st)
                        hip.check(L.es_ddim_rows_update(C.byref(a), hip.current_stream()), 'es_ddim_rows_update')
                        got, stc = x_d.cpu(), int(step_d.item())
                        ref = _ref_rows(x_in, eps[:nslab], noise[st] if with_noise else None, coef[st], mask, x0, tab, kn, st)
                        tag = 'O=%d mask=%s step=%d slabs=%d noise=%d inc=%d' % (O, mname, st, nslab, with_noise, inc)
                        assert torch.isfinite(got).all(), tag
                        assert torch.equal(got, ref), tag + ': max abs diff %.3e' % (got - ref).abs().max().item()
                        assert stc == st + inc, tag + ': step counter %d' % stc
                        if mask is not None and st == N_TAB - 1:
                            assert torch.equal(got[mask.bool()], x0[mask.bool()]), tag
                        # es_ddim_update on the same inputs: the same bits on the rows that are not kept
                        u = hip.UpdateArgs()
                        u.x, u.eps, u.coef, u.step = x2_d.data_ptr(), eps_d.data_ptr(), coef_d.data_ptr(), step_d.data_ptr()
                        u.eps_nslab, u.eps_slab_stride, u.coef_stride, u.n, u.inc_step = nslab, n, 5, n, 0
                        if with_noise:
                            u.noise, u.noise_stride = nz_d.data_ptr(), n
                        x2_d.copy_(x_in)
                        step_d.fill_(st)
                        hip.check(L.es_ddim_update(C.byref(u), hip.current_stream()), 'es_ddim_update')
                        free = torch.ones(O, dtype=torch.bool) if mask is None else ~mask.bool()
                        assert torch.equal(x2_d.cpu()[free], got[free]), tag + ': differs from es_ddim_update'
                        checked += 1
    assert checked == 72
    # the two halves really differ on these inputs, and so do the runs with and without noise
    r0 = _ref_rows(x_in, eps[:1], None, coef[0], masks['zeros'], x0, tab, kn, 0)
    r1 = _ref_rows(x_in, eps[:1], None, coef[0], torch.ones(O), x0, tab, kn, 0)
    r2 = _ref_rows(x_in, eps[:1], noise[0], coef[0], None, x0, tab, kn, 0)
    assert not torch.equal(r0, r1) and not torch.equal(r0, r2)


# ------------------------------------------------------------------------------------------------ the denoisers of the loop tests
def _net(mc, ctx, prefix):
    from echoscene_amd.model.unet import UNet1DModel
    kw = dict(escfg.layout_denoiser_kwargs(mc))
    kw['concat_dim'] = kw['crossattn_dim'] = ctx
    net = UNet1DModel(**kw)
    synth.seeded_fill_(net, prefix=prefix)
    return net


@pytest.fixture(scope='module')
def tiny(dev):
    """the model of layout_loop_tiny with T = 1000 trained timesteps: the default denoiser and, on ITS packed weights, DDIM denoisers
    by (steps, eta), built once and shared by the loop tests"""
    from echoscene_amd.samplers import LayoutDenoiser
    net = _net(128, 128, 'unet1d_tiny.')
    dk = escfg.layout_diffusion_kwargs(1000)
    base = LayoutDenoiser(net, dk, dev)
    made = {}

    def ddim(S, eta=0.0):
        if (S, eta) not in made:
            made[(S, eta)] = LayoutDenoiser(net, dk, dev, sampler='ddim', steps=S, eta=eta, weights=base.w)
        return made[(S, eta)]
    g = load_golden('layout_ddim_tiny')
    return dict(base=base, ddim=ddim, g=g, oe=g['obj_embed'], triples=g['triples'], noise=g['noise'])


# ------------------------------------------------------------------------------------------------ 2: loops against the goldens
@pytest.mark.parametrize('tag,S,eta', [('S4', 4, 0.0), ('S5', 5, 0.0), ('S4_eta07', 4, 0.7)])
def test_layout_ddim_tiny_vs_reference_golden_every_iteration(dev, tiny, tag, S, eta):
    t = tiny
    den, g = t['ddim'](S, eta), t['g']
    assert den.n_iter == S and den.T == 1000 and den.w is t['base'].w
    assert tuple(den.temb.shape) == (S, 128) and den.tables['emb_all'].shape[0] == S          # S-row tables of its own
    assert [int(v) for v in den.sched.timesteps] == g[tag + '_calls'].tolist()
    for i in range(S):
        x = den.sample(t['oe'], t['triples'], t['noise'][:S + 1], n_steps=i + 1)
        _bar(x, g[tag + '_states'][i], '%s after iteration %d' % (tag, i))
    st = den._last
    assert tuple(st['noise'].shape) == (S + 1, 8, 8) and st['x0'] is None


def test_layout_ddim_tiny_100_steps_vs_reference_golden(dev, tiny):
    t = tiny
    den = t['ddim'](100)
    x = den.sample(t['oe'], t['triples'], t['noise'][:1])
    _bar(x, t['g']['S100_x_final'], 'S = 100 of T = 1000, tiny width')


def test_layout_ddim_full_width_vs_reference_golden(dev):
    from echoscene_amd.samplers import LayoutDenoiser
    g, gf = load_golden('layout_ddim_full'), load_golden('unet1d_full')
    den = LayoutDenoiser(_net(512, 1280, 'unet1d_full.'), escfg.layout_diffusion_kwargs(1000), dev, sampler='ddim', steps=10)
    assert [int(v) for v in den.sched.timesteps] == g['calls'].tolist()
    x1 = den.sample(gf['loop_obj_embed'], gf['loop_triples'], g['x_T'][None], n_steps=1)
    _bar(x1, g['x_iter0'], 'full width after iteration 0')
    x = den.sample(gf['loop_obj_embed'], gf['loop_triples'], g['x_T'][None])
    _bar(x, g['x_final'], 'full width, S = 10')


# ------------------------------------------------------------------------------------------------ 3: the masked loop
@pytest.fixture(scope='module')
def kept(tiny):
    g = load_golden('layout_ddim_keep_tiny')
    keep = g['keep'].long()
    xs, qs = [int(v) for v in g['seeds']]
    x0 = torch.zeros(4, 8)
    x0[keep] = _rnd((len(keep), 8), xs, 0.5)
    table = torch.stack([_rnd((4, 8), qs + k) for k in range(4)])
    assert torch.equal(x0, g['x0']) and torch.equal(table, g['keep_noise'])
    mask = torch.zeros(4)
    mask[keep] = 1.0
    return dict(g=g, keep=keep, gen=(mask == 0).nonzero().flatten(), x0=x0, table=table, mask=mask, oe=g['obj_embed'],
                triples=g['triples'], noise=g['x_T'][None], den=tiny['ddim'](4))


def test_masked_layout_ddim_vs_reference_golden(dev, kept):
    k = kept
    den, g, gen, keep = k['den'], k['g'], k['gen'], k['keep']
    a = (k['oe'], k['triples'], k['noise'])
    st = den.stage(*a, k['x0'], k['mask'], k['table'])
    first = st['x'].clone()
    _bar(first[keep], g['img_first'][keep], 'kept rows in front of iteration 0')
    assert torch.equal(first.cpu()[gen], g['x_T'][gen])
    tab = den.keep_tab.cpu()
    assert torch.equal(first.cpu()[keep], (tab[0, 0] * k['x0'] + tab[0, 1] * k['table'][0])[keep])     # q_sample at ts[0], this table's bits
    x = den.sample(*a, x0=k['x0'], mask=k['mask'], keep_noise=k['table'])
    _bar(x[gen], g['x_final'][gen], 'generated rows of the masked loop')
    assert torch.equal(x.cpu()[keep], k['x0'][keep]), 'kept rows are x0, bit for bit'
    plain = den.sample(*a)
    _bar(plain, g['x_final_unmasked'], 'the unmasked run of the same inputs')
    big = _rnd((4, 8), 9, 2.0)
    assert torch.equal(den.sample(*a, x0=big, mask=torch.zeros(4), keep_noise=k['table']), plain), 'an all-zero mask: nothing is kept'
    assert torch.equal(den.sample(*a, x0=big, mask=torch.ones(4), keep_noise=k['table']).cpu(), big)
    # the kept nodes are context
    assert float((x[gen] - plain[gen]).abs().amax(dim=1).min()) > 1e-3
    # stopped early: the kept rows hold the NEXT iteration's forward-noised value
    x3 = den.sample(*a, n_steps=3, x0=k['x0'], mask=k['mask'], keep_noise=k['table'])
    assert torch.equal(x3.cpu()[keep], (tab[3, 0] * k['x0'] + tab[3, 1] * k['table'][3])[keep])
    with pytest.raises(ValueError):
        den.sample(*a, x0=k['x0'], mask=k['mask'], keep_noise=k['table'][:3])
    with pytest.raises(ValueError, match='clip_denoised'):
        den.sample(*a, clip_denoised=True)


# ------------------------------------------------------------------------------------------------ 4: bit-for-bit identities
def test_graph_eager_repeat_and_the_default_loop_untouched(dev, tiny):
    from echoscene_amd import hip
    from test_hip_keep import op_signature
    t = tiny
    a = (t['oe'], t['triples'])
    base, den = t['base'], t['ddim'](4, 0.7)
    nz = synth.layout_noise(8, 8, 1000, seed=7)
    before = base.sample(*a, nz, n_steps=30)
    x = den.sample(*a, t['noise'][:5], use_graph=True)
    assert torch.equal(den.sample(*a, t['noise'][:5], use_graph=False), x)
    assert torch.equal(den.sample(*a, t['noise'][:5], use_graph=True), x)
    den._last['plan'].poison_scratch()
    assert torch.equal(den.sample(*a, t['noise'][:5]), x)
    assert torch.equal(base.sample(*a, nz, n_steps=30), before), "the default 'ddpm' run after a DDIM run"
    assert not torch.equal(t['ddim'](4).sample(*a, t['noise'][:5]), x), 'eta = 0.7 reads the draws'
    # the plans the denoisers really run: the same ops with the last one replaced, and as many launches
    pb, pd = base._plan_for(*a)['plan'], den._plan_for(*a)['plan']
    sb, sd = op_signature(pb), op_signature(pd)
    assert len(sb) == len(sd) and sb[:-1] == sd[:-1] and sb[-1][0] == hip.OP_DDPM and sd[-1][0] == hip.OP_DDIM_ROWS
    assert pb.n_launches == pd.n_launches and all(s[0] != hip.OP_DDIM_ROWS for s in sb)
    assert base.n_iter == base.T == 1000 and tuple(base.temb.shape) == (1000, 128)


@pytest.mark.parametrize('S_lay,eta,r', [(4, 0.0, 1), (8, 0.7, 2), (2, 0.0, 0)])
def test_fused_call_equals_the_two_loops_run_separately(dev, tiny, S_lay, eta, r):
    """sample_layout_and_shape with a DDIM layout denoiser next to a 4-step shape denoiser: r = n_iter_layout // n_iter_shape layout
    steps per replay (r = 0: the unfused branch)"""
    from echoscene_amd.samplers import sample_layout_and_shape, fused_iterations
    from test_hip_keep import _shape
    t = tiny
    lay, shp = t['ddim'](S_lay, eta), _shape(dev)
    assert fused_iterations(lay.n_iter, shp.S)[0] == r
    uc, n1 = _rnd((8, 1, 64), 52), synth.shape_noise(seed=7)
    nz = synth.layout_noise(8, 8, S_lay, seed=11)
    x_alone = lay.sample(t['oe'], t['triples'], nz)
    z_alone = shp.sample(uc, t['triples'], noise1=n1)
    x, z = sample_layout_and_shape(lay, shp, t['oe'], t['triples'], uc, layout_noise=nz, shape_noise=n1)
    assert torch.equal(x, x_alone), 'max abs diff %.3e' % (x - x_alone).abs().max().item()
    assert torch.equal(z, z_alone)


def test_seeded_call_draws_in_the_documented_order(dev, kept, tiny):
    """keep table [n_iter, O * 8], then noise [n_iter + 1, O, 8], each in one call"""
    k = kept
    den = tiny['ddim'](4, 0.7)
    a = (k['oe'], k['triples'])
    torch.manual_seed(5)
    x = den.sample(*a, x0=k['x0'], mask=k['mask'])
    torch.manual_seed(5)
    kn = torch.empty(4, 4 * 8, device=dev).normal_()
    nz = torch.empty(5, 4, 8, device=dev).normal_()
    x2 = den.sample(*a, nz, x0=k['x0'], mask=k['mask'], keep_noise=kn.reshape(4, 4, 8))
    assert torch.equal(x, x2)
    torch.manual_seed(5)
    y = den.sample(*a)
    torch.manual_seed(5)
    nz = torch.empty(5, 4, 8, device=dev).normal_()
    assert torch.equal(y, den.sample(*a, nz))


# ------------------------------------------------------------------------------------------------ 5: the model file
def test_layout_ddim_model_files(dev, tiny, kept, tmp_path):
    from echoscene_amd import hip
    L = hip.lib()
    p = lambda v: C.c_void_p(v.data_ptr())
    t, k = tiny, kept
    den = t['ddim'](4, 0.7)
    nz = t['noise'][:5].contiguous().to(dev)
    ref = den.sample(t['oe'], t['triples'], nz)
    path = str(tmp_path / 'layout_ddim.esm')
    den.save_model(path, t['oe'], t['triples'])
    m = L.es_model_load(path.encode())
    assert m, L.es_last_error()
    try:
        out = torch.full((8, 8), float('nan'), device=dev)
        hip.check(L.es_layout_sample(C.c_void_p(m), p(nz), 5, 4, p(out), hip.current_stream()), 'es_layout_sample')
        torch.cuda.synchronize()
        assert torch.equal(out, ref), 'max abs diff %.3e' % (out - ref).abs().max().item()
        assert L.es_model_run(C.c_void_p(m), 2, 3, hip.current_stream()) != 0 and b'schedule' in L.es_last_error()
        x0, mk, kn = (v.contiguous().to(dev) for v in (torch.zeros(8, 8), torch.zeros(8), torch.zeros(4, 8, 8)))
        assert L.es_layout_sample_keep(C.c_void_p(m), p(nz), 5, 4, p(x0), p(mk), p(kn), p(out), hip.current_stream()) != 0   # no mask in this plan
    finally:
        L.es_model_free(C.c_void_p(m))
    # keep=True
    den = k['den']
    nz = k['noise'].contiguous().to(dev).repeat(5, 1, 1)
    ref = den.sample(k['oe'], k['triples'], nz, x0=k['x0'], mask=k['mask'], keep_noise=k['table'])
    path = str(tmp_path / 'layout_ddim_keep.esm')
    den.save_model(path, k['oe'], k['triples'], keep=True)
    m = L.es_model_load(path.encode())
    assert m, L.es_last_error()
    try:
        x0, mk, kn = (v.contiguous().to(dev) for v in (k['x0'], k['mask'], k['table']))
        out = torch.full((4, 8), float('nan'), device=dev)
        hip.check(L.es_layout_sample_keep(C.c_void_p(m), p(nz), 5, 4, p(x0), p(mk), p(kn), p(out), hip.current_stream()),
                  'es_layout_sample_keep')
        torch.cuda.synchronize()
        assert torch.equal(out, ref), 'max abs diff %.3e' % (out - ref).abs().max().item()
        assert torch.equal(out.cpu()[k['keep']], k['x0'][k['keep']])
        nz6 = torch.zeros(6, 4, 8, device=dev)
        assert L.es_layout_sample_keep(C.c_void_p(m), p(nz6), 6, 5, p(x0), p(mk), p(kn), p(out), hip.current_stream()) != 0
        assert b'schedule' in L.es_last_error()
    finally:
        L.es_model_free(C.c_void_p(m))


# ------------------------------------------------------------------------------------------------ 6: the scene calls
@pytest.mark.parametrize('typ,fam', [('echolayout', 'lay_'), ('echoscene', 'sc_')])
def test_sgdiff_layout_ddim_vs_reference_golden(typ, fam):
    """sample_box_and_shape(..., layout_sampler='ddim', layout_steps=4) against scene_layout_ddim_tiny (the reference's scene call with
    its layout loop replaced by its DDIMSampler through the adapter) at the scene calls' 1e-4 of the tensor scale; with keep_box_nodes
    the kept rows are the caller's bits; the same call without the keywords is what it was, before and after; the denoisers share
    one set of packed weights and invalidate() drops them all."""
    from test_hip_keep import _build_sgdiff, _rel
    g = load_golden('scene_layout_ddim_tiny')
    objs, triples = g['objs'], g['triples']
    O = objs.shape[0]
    tf, rf = synth.synthetic_features(O, triples.shape[0], seed=9)
    a = (objs.cuda(), triples.cuda(), tf.cuda(), rf.cuda())
    cat = lambda d: torch.cat([d['sizes'], d['translations'], d['angles']], 1)
    ln = synth.layout_noise(O, 8, 100, seed=7)
    m = _build_sgdiff(typ)
    kw = dict(gen_shape=False) if typ == 'echoscene' else {}
    before = m.sample_box_and_shape(*a, layout_noise=ln, **kw)
    d = m.sample_box_and_shape(*a, layout_noise=ln[:5], layout_sampler='ddim', layout_steps=4, **kw)
    for k in ('sizes', 'translations', 'angles'):
        e = _rel(d[k], g[fam + k])
        print('scene layout ddim, %s %s: rel err %.2e' % (typ, k, e))
        assert e < 1e-4, k
    Ld = m.diff.LayoutDiff
    dd = Ld._denoiser('ddim', 4)
    assert dd is Ld._dens[('ddim', 4, 0.0)] and dd.w is Ld._denoiser().w and dd.n_iter == 4 and Ld._denoiser().n_iter == 100
    assert [int(v) for v in dd.sched.timesteps] == g[fam + 'calls'].tolist()
    assert torch.equal(cat(m.sample_box_and_shape(*a, layout_noise=ln, **kw)), cat(before)), 'the default call after a DDIM call'
    # kept boxes: the caller's bits
    keep = [0, 2, 5]
    boxes = _rnd((len(keep), 8), 73, 0.5)
    dk = m.sample_box_and_shape(*a, layout_noise=ln[:5], layout_sampler='ddim', layout_steps=4, keep_box_nodes=keep, keep_boxes=boxes,
                                keep_box_noise=_rnd((4, O, 8), 1970), **kw)
    assert torch.equal(cat(dk).cpu()[keep], boxes) and not torch.equal(cat(dk), cat(d))
    # the editing calls take the keywords too; eta != 0 is another denoiser on the same weights
    np.random.seed(5)
    k2, d2 = m.sample_boxes_and_shape_with_changes(*a, *a, [1], layout_noise=ln[:5], layout_sampler='ddim', layout_steps=4, layout_eta=0.5, **kw)
    assert tuple(cat(d2).shape) == (O, 8) and bool(torch.isfinite(cat(d2)).all())
    assert ('ddim', 4, 0.5) in Ld._dens and Ld._dens[('ddim', 4, 0.5)].w is dd.w
    with pytest.raises(ValueError, match='layout_'):
        m.sample_box_and_shape(*a, layout_noise=ln, layout_steps=4, **kw)
    if typ == 'echoscene':
        # shapes generated too: the fused graph with the DDIM plan as its side branch (4 layout steps next to 4 shape steps) -- the same boxes
        n1 = synth.shape_noise(seed=7)
        ds = m.sample_box_and_shape(*a, gen_shape=True, layout_noise=ln[:5], shape_noise=n1, layout_sampler='ddim', layout_steps=4)
        assert torch.equal(cat(ds), cat(d)) and tuple(ds['shapes'].shape) == (O, 1, 64, 64, 64)
        dp = m.sample_box_and_shape(*a, gen_shape=True, layout_noise=ln[:5], shape_noise=n1, layout_sampler='ddim', layout_steps=4,
                                    shape_sampler='plms', shape_steps=4)
        assert torch.equal(cat(dp), cat(d))
    m.diff.invalidate()
    assert Ld._den is None and Ld._dens == {}
    assert torch.equal(cat(m.sample_box_and_shape(*a, layout_noise=ln, **kw)), cat(before))
