"""GPU tests of PLMS shape sampling (``ShapeDenoiser(sampler='plms')``, ``shape_sampler=`` / ``shape_steps=`` of the scene calls) against
goldens made by the reference's own PLMSSampler (tests/golden/make_golden_plms.py), and of the three kernels alone against a torch-CPU
restatement.  Bars are the project's: 2e-2 of the tensor scale on the fp16-operand route (``_rel`` of
test_hip_keep.py), atol = rtol = 1e-3 on the 'fp32x' route (test_shape_100_ddim_steps_fp32_operand_route_vs_reference)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from conftest import load_golden
from echoscene_amd import synth

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda')


def _rnd(shape, seed, scale=1.0):
    return torch.from_numpy((np.random.RandomState(seed).standard_normal(shape) * scale).astype(np.float32))


# ------------------------------------------------------------------------------------------------ the three kernels alone
def _ddim_cpu(x, e, c):
    """get_x_prev_and_pred_x0 at sigma = 0, one torch op per arithmetic op (fp32 on the CPU: nothing is contracted)"""
    t = torch.mul(e, c[0])
    t = torch.sub(x, t)
    px0 = torch.div(t, torch.full_like(t, float(c[1])))
    a = torch.mul(px0, c[2])
    b = torch.mul(e, c[3])
    return torch.add(a, b)


def _div(t, d):
    return torch.div(t, torch.full_like(t, d))


def _eprime_cpu(e, h1, h2, h3, st):
    if st <= 1:
        return _div(torch.sub(torch.mul(e, 3.0), h1), 2.0)
    if st == 2:
        t = torch.sub(torch.mul(e, 23.0), torch.mul(h1, 16.0))
        return _div(torch.add(t, torch.mul(h2, 5.0)), 12.0)
    t = torch.sub(torch.mul(e, 55.0), torch.mul(h1, 59.0))
    t = torch.add(t, torch.mul(h2, 37.0))
    return _div(torch.sub(t, torch.mul(h3, 9.0)), 24.0)


@pytest.mark.parametrize('nslab', [1, 2])
def test_plms_kernels_vs_torch_restatement(dev, nslab):
    """es_plms_first_a / es_plms_first_b / es_plms_update at n = 4 x 12288 (192 workgroups), eps as 1 and 2 slabs, counter values 0..5:
    x, the ring, xsave and the counter equal the restatement bit for bit.  Counters 1, 2, 3 are the three orders; 3, 4, 5 walk the ring
    once round (slot st % 3 is read as h3 and then overwritten with e, not e'); coefficient row st is used."""
    from echoscene_amd import hip
    from echoscene_amd.schedules import ShapeSchedule
    L = hip.lib()
    n = 4 * 12288
    coef_h = ShapeSchedule(8).coef                               # [8, 4]: rows 0..5 are used
    coef = coef_h.to(dev)
    x_h, ring_h, xs_h = _rnd((n,), 1, 3.0), _rnd((3, n), 2), _rnd((n,), 3)
    slabs_h = _rnd((nslab, n), 4)
    e_h = slabs_h[0].clone()
    for j in range(1, nslab):
        e_h = torch.add(e_h, slabs_h[j])
    slabs = slabs_h.to(dev)
    step = torch.zeros(1, dtype=torch.int32, device=dev)

    def args(x, ring, xsave):
        a = hip.PlmsArgs()
        a.x, a.eps, a.eps_nslab, a.eps_slab_stride = x.data_ptr(), slabs.data_ptr(), nslab, n
        a.coef, a.coef_stride, a.n, a.step, a.inc_step = coef.data_ptr(), 4, n, step.data_ptr(), 1
        a.ring, a.ring_stride, a.xsave = ring.data_ptr(), n, xsave.data_ptr()
        return a
    s = hip.current_stream()
    # first-a at counter 0: xsave = x, ring[0] = e, x = ddim(x, e, row 0), counter 1
    x, ring, xsave = x_h.to(dev), ring_h.to(dev), xs_h.to(dev)
    hip.check(L.es_plms_first_a(C.byref(args(x, ring, xsave)), s), 'es_plms_first_a')
    torch.cuda.synchronize()
    want_ring = ring_h.clone()
    want_ring[0] = e_h
    assert torch.equal(x.cpu(), _ddim_cpu(x_h, e_h, coef_h[0])) and torch.equal(xsave.cpu(), x_h)
    assert torch.equal(ring.cpu(), want_ring) and int(step.item()) == 1
    # first-b at counter 1 (left alone): x = ddim(xsave, (ring[0] + e) / 2, row 0); ring and xsave unchanged
    x, ring, xsave = x_h.to(dev), ring_h.to(dev), xs_h.to(dev)
    hip.check(L.es_plms_first_b(C.byref(args(x, ring, xsave)), s), 'es_plms_first_b')
    torch.cuda.synchronize()
    ep = _div(torch.add(ring_h[0], e_h), 2.0)
    assert torch.equal(x.cpu(), _ddim_cpu(xs_h, ep, coef_h[0]))
    assert torch.equal(ring.cpu(), ring_h) and torch.equal(xsave.cpu(), xs_h) and int(step.item()) == 1
    # the steady update at every counter value
    for st in range(0, 6):
        x, ring = x_h.to(dev), ring_h.to(dev)
        step.fill_(st)
        hip.check(L.es_plms_update(C.byref(args(x, ring, xsave)), s), 'es_plms_update')
        torch.cuda.synchronize()
        h1, h2, h3 = ring_h[(st + 2) % 3], ring_h[(st + 1) % 3], ring_h[st % 3]
        ep = _eprime_cpu(e_h, h1, h2, h3, st)                      # (counter 0 is never planned: it takes the order of counter 1)
        want_ring = ring_h.clone()
        want_ring[st % 3] = e_h
        assert torch.equal(x.cpu(), _ddim_cpu(x_h, ep, coef_h[st])), st
        assert torch.equal(ring.cpu(), want_ring), st
        assert int(step.item()) == st + 1
    a = args(x, ring, xsave)
    a.inc_step = 0
    step.fill_(2)
    hip.check(L.es_plms_update(C.byref(a), s), 'es_plms_update')
    torch.cuda.synchronize()
    assert int(step.item()) == 2


# ------------------------------------------------------------------------------------------------ the loop against the reference
def _check_states(den, g, S, use_graph=True, **kw):
    """the state after every iteration against the golden's subsampled states (n_steps counts iterations); returns the worst"""
    from test_hip_keep import _rel
    noise1 = synth.shape_noise(seed=7)
    worst = 0.0
    for k in range(1, S + 1):
        zk = den.sample(g['uc_s'], g['triples'], noise1, n_steps=k, use_graph=use_graph, **kw)
        sub = g['S%d_states_sub' % S][k - 1] if ('S%d_states_sub' % S) in g else g['states_sub'][k - 1]
        e = _rel(zk[:, :, ::4, ::4, ::4], sub)
        print('  after iteration %d of %d: rel err %.3e' % (k - 1, S, e))
        worst = max(worst, e)
    return worst


@pytest.mark.parametrize('use_graph', [False, True])
@pytest.mark.parametrize('S', [4, 5])
def test_plms_tiny_vs_reference_golden(dev, S, use_graph):
    """ShapeDenoiser(sampler='plms').sample against the reference's PLMSSampler.sample(S) (S = 4: every order once; S = 5: a ring slot
    overwritten and read back as h1): final latents and the state after every iteration at the fp16 route's 2e-2; two runs and a run
    after poison_scratch() give the same bits; a sampler='ddim' run afterwards on the same object reproduces ddim_tiny and its plan
    is, op for op, the plan of the parent commit (tests/golden/shape_plan_ops_tiny.json)."""
    from test_hip_keep import _shape, _rel, op_signature
    from echoscene_amd import hip
    g = load_golden('plms_tiny')
    den = _shape(dev, S=S, sampler='plms')
    noise1 = synth.shape_noise(seed=7)
    z = den.sample(g['uc_s'], g['triples'], noise1, use_graph=use_graph)
    e = _rel(z, g['S%d_z_final' % S])
    print('plms tiny, S = %d (%d evaluations), use_graph=%s: latent vs fp32 reference golden: rel err %.3e' % (S, S + 1, use_graph, e))
    assert e < 2e-2
    assert _check_states(den, g, S, use_graph=use_graph) < 2e-2
    assert torch.equal(den.sample(g['uc_s'], g['triples'], noise1, use_graph=use_graph), z)
    st = den._plan_for(g['uc_s'], g['triples'], None)
    assert st['sampler'] == 'plms' and st['plan'].poison_scratch() > 0       # (first_plan works on the same buffers)
    assert torch.equal(den.sample(g['uc_s'], g['triples'], noise1, use_graph=use_graph), z)
    kinds = [op.kind for op in st['plan']._arr]
    first = [op.kind for op in st['first_plan']._arr]
    assert kinds[-1] == hip.OP_PLMS and hip.OP_DDIM not in kinds and kinds.count(hip.OP_PLMS) == 1
    assert first == kinds[:-1] + [hip.OP_PLMS_FIRST_A] + kinds[:-1] + [hip.OP_PLMS_FIRST_B]
    if S == 4:
        # the DDIM loop on the same object: the old results, the old plan
        gd = load_golden('ddim_tiny')
        z0 = den.sample(g['uc_s'], g['triples'], noise1, use_graph=use_graph, sampler='ddim')
        assert _rel(z0, gd['z_final']) < 2e-2
        assert _rel(z0, g['S4_z_final']) > 4e-2, 'PLMS and DDIM differ by far more than the bar: the golden tells them apart'
        with open(os.path.join(HERE, 'golden', 'shape_plan_ops_tiny.json')) as f:
            parent_ops = json.load(f)
        plain = den._plan_for(g['uc_s'], g['triples'], None, sampler='ddim')
        assert op_signature(plain['plan']) == parent_ops, 'the ddim plan differs from the plan of the parent commit'
        assert op_signature(st['plan'])[:-1] == parent_ops[:-1]
        assert torch.equal(den.sample(g['uc_s'], g['triples'], noise1, use_graph=use_graph), z), 'the DDIM run left the PLMS state alone'


@pytest.mark.parametrize('S', [4, 5])
def test_plms_tiny_fp32x_vs_reference_golden(dev, S):
    """the split-operand route (the reference's arithmetic to ~2^-21 per product) at the fp32 routes' bar, atol = rtol = 1e-3"""
    from test_hip_keep import _shape
    g = load_golden('plms_tiny')
    den = _shape(dev, S=S, sampler='plms', precision='fp32x')
    z = den.sample(g['uc_s'], g['triples'], synth.shape_noise(seed=7)).cpu()
    zr = g['S%d_z_final' % S]
    print('plms tiny fp32x, S = %d: max abs err %.3e (|z| max %.2f)' % (S, (z - zr).abs().max().item(), zr.abs().max().item()))
    assert torch.allclose(z, zr, atol=1e-3, rtol=1e-3)


def _keep_inputs(g, O=4):
    xs, qs = [int(v) for v in g['seeds']]
    x0 = _rnd((O, 3, 16, 16, 16), xs, 0.6)
    table = torch.stack([_rnd((O, 3, 16, 16, 16), qs + k) for k in range(4)])
    mask = torch.zeros(O)
    mask[g['keep'].long()] = 1.0
    return x0, mask, table


def test_plms_keep_tiny_vs_reference_golden(dev):
    """PLMS with kept shapes against PLMSSampler.sample(mask=, x0=) with q_sample's draws injected: the blend runs once per iteration,
    before the FIRST evaluation; the blended state before iteration 0 is ddim_keep_tiny's img_first bit for bit (the same blend); an
    all-zero mask is bit-equal to the unmasked PLMS run."""
    from test_hip_keep import _shape, _rel
    from echoscene_amd import hip
    g = load_golden('plms_keep_tiny')
    x0, mask, table = _keep_inputs(g)
    den = _shape(dev, sampler='plms')
    noise1 = synth.shape_noise(seed=7)
    kw = dict(x0=x0, mask=mask, keep_noise=table)
    z = den.sample(g['uc_s'], g['triples'], noise1, **kw)
    e = _rel(z, g['z_final'])
    print('plms keep tiny (4 iterations, nodes %s kept): latent vs fp32 reference golden: rel err %.3e' % (g['keep'].tolist(), e))
    assert e < 2e-2
    assert _check_states(den, g, 4, **kw) < 2e-2
    assert torch.equal(den.sample(g['uc_s'], g['triples'], noise1, **kw), z)
    st = den._plan_for(g['uc_s'], g['triples'], None, keep=True)
    kinds = [op.kind for op in st['plan']._arr]
    first = [op.kind for op in st['first_plan']._arr]
    assert kinds[0] == hip.OP_DDIM_BLEND and kinds[-1] == hip.OP_PLMS
    assert first.count(hip.OP_DDIM_BLEND) == 1 and first[0] == hip.OP_DDIM_BLEND, 'one blend per iteration, before the first evaluation'
    assert first == kinds[:-1] + [hip.OP_PLMS_FIRST_A] + kinds[1:-1] + [hip.OP_PLMS_FIRST_B]
    # the blend of iteration 0 alone: the plan's first op on the loop's initial state
    from echoscene_amd.plan import Builder
    b = Builder(dev)
    b.ops = [st['first_plan']._arr[0]]
    b.keep = [st['first_plan']]
    blend = b.finish()
    st['x'].copy_(noise1.to(dev).expand(4, 3, 16, 16, 16))
    st['step'].zero_()
    blend.run()
    torch.cuda.synchronize()
    assert torch.equal(st['x'].cpu(), load_golden('ddim_keep_tiny')['img_first']) and torch.equal(st['x'].cpu(), g['img_first'])
    z_plain = den.sample(g['uc_s'], g['triples'], noise1)
    zz = den.sample(g['uc_s'], g['triples'], noise1, x0=x0, mask=torch.zeros(4), keep_noise=table)
    assert torch.equal(zz, z_plain), 'an all-zero mask: the blend touches nothing'
    assert not torch.equal(z, z_plain)


@pytest.mark.parametrize('masked', [False, True])
def test_plms_shards_equal_unsharded_bitwise(dev, masked):
    """The PLMS loop sharded over 2 emulated ranks (one GPU, simulated all-gather, deterministic mode) == the unsharded run, bit for
    bit, including the second stem -> exchange -> rest pass of iteration 0 (style of test_keep_shards_equal_unsharded_bitwise)."""
    from test_hip_keep import _shape
    g = load_golden('plms_keep_tiny')
    x0, mask, table = _keep_inputs(g)
    uc, triples, noise1, world, nst = g['uc_s'], g['triples'], synth.shape_noise(seed=7), 2, 4
    kw = dict(x0=x0, mask=mask, keep_noise=table) if masked else {}
    z_ref = _shape(dev, deterministic=True, sampler='plms').sample(uc, triples, noise1, n_steps=nst, **kw)
    shards = [_shape(dev, rank=r, world=world, deterministic=True, sampler='plms') for r in range(world)]
    for sh in shards:
        st = sh._plan_for(uc, triples, None, keep=masked)
        if masked:
            world_, sh.world = sh.world, 1               # (fill this rank's rows from the given table: no collective draw)
            sh._fill_keep(st, x0, mask, table)
            sh.world = world_
        st['x'].copy_(noise1.to(dev).expand(st['hi'] - st['lo'], 3, 16, 16, 16))
        sh._cur, sh._use_graph = st, True
        assert sh.step_graph() is None
    n_exchanges = 0
    for i in range(nst):
        assert [sh.passes(i) for sh in shards] == [2 if i == 0 else 1] * world
        for p in range(shards[0].passes(i)):
            codes = torch.cat([sh.codes_local(i, p)[:sh._cur['hi'] - sh._cur['lo']].clone() for sh in shards], 0)
            n_exchanges += 1
            for sh in shards:
                sh.step(i, codes, p)
    assert n_exchanges == nst + 1
    z = torch.cat([sh.latents_local() for sh in shards], 0)
    assert torch.equal(z, z_ref), 'max abs diff %.3e' % (z - z_ref).abs().max().item()
    if masked:
        assert not torch.equal(z_ref, _shape(dev, deterministic=True, sampler='plms').sample(uc, triples, noise1, n_steps=nst))


def test_plms_constructor_errors(dev):
    from test_hip_keep import _shape
    with pytest.raises(ValueError, match='ddim_eta must be 0 for PLMS'):
        _shape(dev, sampler='plms', ddim_eta=0.5)
    with pytest.raises(ValueError, match='at least 2 timesteps'):
        _shape(dev, S=1, sampler='plms')
    with pytest.raises(ValueError):
        _shape(dev, sampler='heun')
    den = _shape(dev, ddim_eta=0.5)
    g = load_golden('plms_tiny')
    with pytest.raises(ValueError, match='ddim_eta must be 0 for PLMS'):
        den.sample(g['uc_s'], g['triples'], synth.shape_noise(seed=7), sampler='plms')
    with pytest.raises(NotImplementedError):
        _shape(dev, sampler='plms').save_model('/nonexistent/plms.esm', g['uc_s'], g['triples'])


# ------------------------------------------------------------------------------------------------ the fused loop
def test_fused_loop_with_plms_equals_the_separate_loops(dev):
    """sample_layout_and_shape with a PLMS shape loop (S = 4, T = 100: iteration 0 unfused, three fused replays of 25 layout steps each,
    25 left-over layout steps) == LayoutDenoiser.sample and ShapeDenoiser.sample run separately, both bit for bit -- the standard
    test_fused_graph_with_kept_boxes applies to DDIM; the DDIM fused call on the same objects is unchanged by it."""
    from echoscene_amd.samplers import sample_layout_and_shape
    from test_hip_keep import _shape
    from test_hip_rows import _layout
    gp = load_golden('layout_loop_tiny')
    lay = _layout(dev, 128, 128, 'unet1d_tiny.', 100)
    noise = synth.layout_noise(8, 8, 100, seed=7)
    uc, n1 = _rnd((8, 1, 64), 52), synth.shape_noise(seed=7)
    oe, triples = gp['obj_embed'], gp['triples']
    x_alone = lay.sample(oe, triples, noise)
    shp = _shape(dev, sampler='plms')
    z_alone = shp.sample(uc, triples, n1)
    x, z = sample_layout_and_shape(lay, shp, oe, triples, uc, layout_noise=noise, shape_noise=n1)
    assert torch.equal(x, x_alone), 'max abs diff %.3e' % (x - x_alone).abs().max().item()
    assert torch.equal(z, z_alone), 'max abs diff %.3e' % (z - z_alone).abs().max().item()
    x2, z2 = sample_layout_and_shape(lay, shp, oe, triples, uc, layout_noise=noise, shape_noise=n1, use_graph=False)
    assert torch.equal(x2, x_alone) and torch.equal(z2, z_alone)
    # per-call override on a DDIM denoiser, and the DDIM fused call before and after
    sd = _shape(dev)
    xd, zd = sample_layout_and_shape(lay, sd, oe, triples, uc, layout_noise=noise, shape_noise=n1)
    x3, z3 = sample_layout_and_shape(lay, sd, oe, triples, uc, layout_noise=noise, shape_noise=n1, shape_sampler='plms')
    assert torch.equal(x3, x_alone) and torch.equal(z3, z_alone)
    xd2, zd2 = sample_layout_and_shape(lay, sd, oe, triples, uc, layout_noise=noise, shape_noise=n1)
    assert torch.equal(xd, xd2) and torch.equal(zd, zd2) and torch.equal(zd, sd.sample(uc, triples, n1)) and not torch.equal(zd, z)


# ------------------------------------------------------------------------------------------------ the public interface
def test_sgdiff_plms_vs_composed_reference_golden():
    """sample_box_and_shape(shape_sampler='plms', shape_steps=4) against scene_plms_tiny (the reference's scene call with its rel2shape
    composed from PLMSSampler -> decode_no_quant); bars of test_sgdiff_keep_shapes_vs_composed_reference_golden: boxes 1e-4, latents
    2e-2, the SDF as a distribution.  A call without the keywords gives the same bits before and after (no state leaks between the
    samplers) and still meets scene_e2e_tiny; the keywords reach the editing calls and combine with kept shapes; the ValueErrors."""
    from test_hip_keep import _build_sgdiff, _rel
    g = load_golden('scene_plms_tiny')
    objs, triples = g['objs'], g['triples']
    O = objs.shape[0]
    tf, rf = synth.synthetic_features(O, triples.shape[0], seed=9)
    m = _build_sgdiff('echoscene')
    S = m.diff.ShapeDiff
    assert S.shape_sampler == 'ddim' and S.ddim_steps == 4
    a = (objs.cuda(), triples.cuda(), tf.cuda(), rf.cuda())
    kw = dict(layout_noise=synth.layout_noise(O, 8, 100, seed=7), shape_noise=synth.shape_noise(seed=7))
    d0 = m.sample_box_and_shape(*a, gen_shape=True, **kw)
    z0 = S.gen_z.clone()
    d = m.sample_box_and_shape(*a, gen_shape=True, shape_sampler='plms', shape_steps=4, **kw)
    z_plms = S.gen_z.clone()
    # rel2shape takes the keywords too: the unfused loop on the same inputs gives the fused call's latents bit for bit
    sdf_u = S.rel2shape({'obj_cat': a[0], 'triples': a[1], 'c_s': S.rel, 'uc_s': S.uc_rel}, noise=kw['shape_noise'], shape_sampler='plms',
                        shape_steps=4)
    assert torch.equal(S.gen_z, z_plms) and torch.equal(sdf_u, d['shapes'])
    for k in ('sizes', 'translations', 'angles'):
        assert _rel(d[k], g[k]) < 1e-4, k
        assert torch.equal(d[k], d0[k]), 'the layout loop does not depend on the shape sampler'
    ez = _rel(S.gen_z, g['z'])
    print('scene plms: latents after 4 PLMS iterations (5 evaluations) rel err %.2e' % ez)
    assert ez < 2e-2
    got, ref = d['shapes'][:, :, ::4, ::4, ::4].cpu(), g['shapes']
    scale = ref.abs().max().item()
    bad = ((got - ref).abs() > 2e-2 * scale).float().mean().item()
    med = (got - ref).abs().median().item() / scale
    print('scene plms: SDFs vs reference: %.3f%% of samples outside 2e-2, median rel err %.2e' % (100 * bad, med))
    assert bad < (0.03 if O >= 8 else 0.10) and med < 2e-3
    # the default call: the same bits as before the PLMS call, and the DDIM golden
    d1 = m.sample_box_and_shape(*a, gen_shape=True, **kw)
    assert torch.equal(d1['shapes'], d0['shapes']) and torch.equal(S.gen_z, z0) and not torch.equal(z0, g['z'].cuda())
    for k in ('sizes', 'translations', 'angles'):
        assert torch.equal(d1[k], d0[k])
    g0 = load_golden('scene_e2e_tiny')
    got, ref = d0['shapes'][:, :, ::4, ::4, ::4].cpu(), g0['echoscene_shapes']
    assert ((got - ref).abs() > 2e-2 * ref.abs().max().item()).float().mean().item() < 0.03
    # the attribute is the default of the keyword; explicit 'ddim' is the default call
    S.shape_sampler = 'plms'
    d2 = m.sample_box_and_shape(*a, gen_shape=True, **kw)
    assert torch.equal(d2['shapes'], d['shapes'])
    d3 = m.sample_box_and_shape(*a, gen_shape=True, shape_sampler='ddim', **kw)
    assert torch.equal(d3['shapes'], d0['shapes'])
    S.shape_sampler = 'ddim'
    # editing calls and kept shapes take the keywords
    keep = [0, 2]
    sdfs = synth.ellipsoid_sdfs(len(keep), seed=83)
    np.random.seed(5)
    k4, d4 = m.sample_boxes_and_shape_with_changes(*a, *a, [1], gen_shape=True, shape_sampler='plms', shape_steps=4, keep_nodes=keep,
                                                   keep_sdfs=sdfs, **kw)
    assert torch.equal(d4['shapes'][keep].cpu(), sdfs) and torch.isfinite(d4['shapes']).all()
    with pytest.raises(ValueError, match='ddim_eta must be 0 for PLMS'):
        S.rel2shape({'obj_cat': a[0], 'triples': a[1], 'c_s': S.rel, 'uc_s': S.uc_rel}, ddim_eta=0.5, noise=kw['shape_noise'],
                    shape_sampler='plms')
    with pytest.raises(ValueError, match='at least 2 timesteps'):
        m.sample_box_and_shape(*a, gen_shape=True, shape_sampler='plms', shape_steps=1, **kw)
    with pytest.raises(ValueError):
        m.sample_box_and_shape(*a, gen_shape=True, shape_sampler='heun', **kw)
    ml = _build_sgdiff('echolayout')
    with pytest.raises(ValueError):
        ml.sample_box_and_shape(*a, shape_sampler='plms', layout_noise=kw['layout_noise'])
    with pytest.raises(ValueError):
        ml.sample_boxes_and_shape_with_changes(*a, *a, [1], shape_steps=50, layout_noise=kw['layout_noise'])
