"""GPU tests of shape completion: the per-voxel masked-DDIM blend (es_ddim_blend_vox), the range helpers (es_range_mask,
es_partial_shape), the voxel form of the masked shape loop and the ``complete_*`` keywords of the scene calls, against goldens made
by the reference itself (tests/golden/make_golden_complete.py).  Bars: bit equality wherever the arithmetic is the reference's own
(the blend, the masks), the fp16-operand route's 2e-2 relative to the tensor scale for what passes through the denoiser (as
tests/test_hip_keep.py)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from conftest import load_golden
from echoscene_amd import synth
from test_hip_keep import _shape, _rel, _rnd, op_signature, _build_sgdiff
from test_complete_cpu import golden_ranges

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda')


def _ibits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ the kernel alone
def _mixed_mask(V):
    """[V] zeros and ones with lanes (groups of four voxels) of every kind: range 2 at 16^3 (z bounds 3:16: mixed lanes), or a
    hand-made pattern for a small V"""
    if V == 4096:
        return load_golden('partial_shape_ranges')['z_mask'][1].reshape(-1).float()
    m = torch.zeros(V)
    m[0:4] = 1                      # an all-ones lane
    m[5], m[10], m[11], m[12:15], m[19] = 1, 1, 1, 1, 1       # mixed lanes of 1, 2 and 3 ones
    m[V - 1] = 1                    # (lanes 5.. of zeros; the last element)
    return m


@pytest.mark.parametrize('V', [64, 4096])
@pytest.mark.parametrize('case', ['zeros', 'ones', 'mixed'])
def test_blend_vox_bit_exact_vs_host_expression(dev, V, case):
    """es_ddim_blend_vox at O = 3, C = 3 and a step other than 0 against the same expression in torch fp32 on the host (two products,
    one sum), bit for bit; where the mask is 0, x0 and noise hold NaN and x comes back with its own bits.  'mixed': object 0 all zero,
    object 1 all ones, object 2 a mask with lanes of every kind."""
    from echoscene_amd.plan import Builder
    O, Cc, S, st = 3, 3, 4, 2
    stride = O * Cc * V + 8                                    # (a table with padding between the steps' draws)
    mask = torch.zeros(O, V)
    if case == 'ones':
        mask[:] = 1
    elif case == 'mixed':
        mask[1], mask[2] = 1, _mixed_mask(V)
    x = _rnd((O, Cc, V), 21)
    x0 = _rnd((O, Cc, V), 22, 0.6)
    noise = _rnd((S, stride), 23)
    tab = torch.tensor([[0.9, 0.1], [0.8, 0.3], [0.7310585976, 0.6823278069], [0.2, 0.97]])
    keepm = mask.bool()[:, None, :].expand(O, Cc, V)
    nz = noise[st, :O * Cc * V].reshape(O, Cc, V)
    p, q = tab[st, 0] * x0, tab[st, 1] * nz
    want = torch.where(keepm, p + q, x)
    # garbage where the mask is 0: the result may not depend on it
    x0g, noiseg = x0.clone(), noise.clone()
    x0g[~keepm] = float('nan')
    noiseg[:, :O * Cc * V].reshape(S, O, Cc, V)[:, ~keepm] = float('nan')
    noiseg[:, O * Cc * V:] = float('nan')
    b = Builder(dev)
    xd = b.dev(x)
    step = b.buf(1, dtype=torch.int32, zero=True)
    b.blend_vox(xd, b.dev(x0g), b.dev(mask), b.dev(noiseg), b.dev(tab), step)
    plan = b.finish()
    step.fill_(st)
    plan.run()
    torch.cuda.synchronize()
    assert int(step.item()) == st, 'the step counter is read, never advanced'
    got = xd.cpu()
    assert torch.isfinite(got).all()
    assert torch.equal(_ibits(got), _ibits(want)), 'max abs diff %.3e' % (got - want).abs().max().item()
    assert torch.equal(_ibits(got)[~keepm], _ibits(x)[~keepm])
    if case != 'zeros':
        assert not torch.equal(got, x)


def test_range_mask_and_partial_shape_equal_the_reference_bitwise(dev):
    """postprocess.latent_range_mask (es_range_mask) and postprocess.partial_shape (es_partial_shape) against what the reference's
    get_partial_shape produced for the six ranges (partial_shape_ranges), at 16^3 and 64^3: masks bit for bit, shape_part /
    shape_missing on the stored sub-samples bit for bit, their abs-sums"""
    from echoscene_amd.postprocess import latent_range_mask, partial_shape
    g = load_golden('partial_shape_ranges')
    ranges = golden_ranges(g)
    zm = latent_range_mask(ranges, (16, 16, 16), dev)
    assert tuple(zm.shape) == (6, 1, 16, 16, 16) and zm.dtype == torch.float32 and zm.is_cuda
    assert torch.equal(zm[:, 0].cpu(), g['z_mask'].float())
    assert [int(v) for v in zm.flatten(1).sum(1).tolist()] == [2048, 1248, 1040, 0, 4096, 1]
    sdf = synth.ellipsoid_sdfs(2, seed=int(g['sdf_seed'][0])).to(dev)
    # one call for all six ranges x both SDFs: K = 12, one range per grid
    ret = partial_shape(sdf.repeat(6, 1, 1, 1, 1), [r for r in ranges for _ in range(2)])
    assert ret['shape_mask'].dtype == torch.bool and all(ret[k].is_cuda for k in ('shape_part', 'shape_missing', 'shape_mask', 'z_mask'))
    part, miss = ret['shape_part'].cpu().reshape(6, 2, 1, 64, 64, 64), ret['shape_missing'].cpu().reshape(6, 2, 1, 64, 64, 64)
    smask = ret['shape_mask'].cpu().reshape(6, 2, 64 ** 3)
    for k in range(6):
        for o in range(2):
            assert np.array_equal(np.packbits(smask[k, o].numpy()), g['shape_mask_bits'][k].numpy()), (k, o)
        assert torch.equal(part[k][:, :, ::4, ::4, ::4], g['shape_part_sub'][k]), k
        assert torch.equal(miss[k][:, :, ::4, ::4, ::4], g['shape_missing_sub'][k]), k
        assert abs(part[k].double().abs().sum().item() - g['shape_part_abs'][k].item()) <= 1e-9 * g['shape_part_abs'][k].item(), k
        assert abs(miss[k].double().abs().sum().item() - g['shape_missing_abs'][k].item()) <= 1e-9 * g['shape_missing_abs'][k].item(), k
    assert torch.equal(ret['z_mask'][::2, 0].cpu(), g['z_mask'].float())
    # inside the range the SDF itself, outside the fill -- and the complement; another fill value
    m = ret['shape_mask'].cpu().reshape(6, 2, 1, 64, 64, 64)
    s6 = sdf.cpu().expand(6, 2, 1, 64, 64, 64)
    assert torch.equal(part, torch.where(m, s6, torch.tensor(0.2))) and torch.equal(miss, torch.where(m, torch.tensor(0.2), s6))
    r5 = partial_shape(sdf[:1], ranges[2], fill=-0.5)
    assert torch.equal(r5['shape_part'].cpu(), torch.where(m[2, :1], sdf[:1].cpu(), torch.tensor(-0.5)))
    with pytest.raises(ValueError):
        partial_shape(sdf, ranges[:1])
    with pytest.raises(ValueError):
        partial_shape(sdf.cpu(), ranges[:2])


# ------------------------------------------------------------------------------------------------ the loop
def _complete_inputs(g, O=4):
    xs, qs = [int(v) for v in g['seeds']]
    x0 = _rnd((O, 3, 16, 16, 16), xs, 0.6)
    table = torch.stack([_rnd((O, 3, 16, 16, 16), qs + k) for k in range(4)])
    return x0, g['z_mask'].float(), table


@pytest.mark.parametrize('use_graph', [False, True])
def test_ddim_complete_tiny_vs_reference_golden(dev, use_graph):
    """ShapeDenoiser.sample(x0, mask [O, 1, D, H, W], keep_noise) against the reference's DDIMSampler.sample(mask=z_mask, x0=) with
    q_sample's draws injected (node 0 range 1, node 1 all ones, node 2 range 2, node 3 all zero); the blended latent in front of the
    first and the last denoiser is the reference's, bit for bit; all-ones rows are the per-object loop's bits; an all-zero voxel
    mask is the unmasked run's bits; the mask=None and the per-object plans are what they were."""
    from echoscene_amd import hip
    g = load_golden('ddim_complete_tiny')
    x0, vmask, table = _complete_inputs(g)
    assert tuple(vmask.shape) == (4, 1, 16, 16, 16)
    den = _shape(dev)
    noise1 = synth.shape_noise(seed=7)
    a = (g['uc_s'], g['triples'], noise1)
    z = den.sample(*a, use_graph=use_graph, x0=x0, mask=vmask, keep_noise=table)
    e = _rel(z, g['z_final'])
    print('ddim complete tiny (4 steps, voxel mask): latent vs fp32 reference golden: rel err %.3e' % e)
    assert e < 2e-2
    assert torch.equal(den.sample(*a, use_graph=use_graph, x0=x0, mask=vmask[:, 0], keep_noise=table), z), '[O, D, H, W] is the same mask'
    vox = den._plan_for(g['uc_s'], g['triples'], None, keep='vox')
    assert tuple(vox['mask'].shape) == (4, 4096) and vox['plan'].poison_scratch() > 0
    assert torch.equal(den.sample(*a, use_graph=use_graph, x0=x0, mask=vmask, keep_noise=table), z)
    # the blend alone: what the denoiser of the first and of the last step sees
    from echoscene_amd.plan import Builder
    b = Builder(dev)
    x = b.dev(noise1.expand(4, 3, 16, 16, 16))
    step = b.buf(1, dtype=torch.int32, zero=True)
    b.blend_vox(x, b.dev(x0), b.dev(vmask.reshape(4, -1)), b.dev(table.reshape(4, -1)), den.keep_tab, step)
    plan = b.finish()
    plan.run()
    torch.cuda.synchronize()
    assert torch.equal(x.cpu(), g['img_first']), 'q_sample on the voxels with mask 1, the others untouched: bit for bit'
    step.fill_(3)
    x.copy_(g['img_last'].to(dev))
    x[vmask.bool().expand(4, 3, 16, 16, 16)] = 7.0
    plan.run()
    torch.cuda.synchronize()
    assert torch.equal(x.cpu(), g['img_last'])
    # all-ones rows == the per-object masked loop; an all-zero voxel mask == the unmasked loop
    omask = torch.tensor([0.0, 1.0, 0.0, 1.0])
    z_obj = den.sample(*a, use_graph=use_graph, x0=x0, mask=omask, keep_noise=table)
    z_vox = den.sample(*a, use_graph=use_graph, x0=x0, mask=omask.reshape(4, 1, 1, 1, 1).expand(4, 1, 16, 16, 16), keep_noise=table)
    assert torch.equal(z_vox, z_obj), 'max abs diff %.3e' % (z_vox - z_obj).abs().max().item()
    assert not torch.equal(z_obj, z)
    z0 = den.sample(*a, use_graph=use_graph)
    assert torch.equal(den.sample(*a, use_graph=use_graph, x0=x0, mask=torch.zeros(4, 1, 16, 16, 16), keep_noise=table), z0)
    assert _rel(z0, load_golden('ddim_tiny')['z_final']) < 2e-2
    # the plans: mask=None as recorded for the parent commit; per object: es_ddim_blend in front; per voxel: op 28 in front
    plain = den._plan_for(g['uc_s'], g['triples'], None)
    keep = den._plan_for(g['uc_s'], g['triples'], None, keep=True)
    vox = den._plan_for(g['uc_s'], g['triples'], None, keep='vox')
    with open(os.path.join(HERE, 'golden', 'shape_plan_ops_tiny.json')) as f:
        parent_ops = json.load(f)
    sig, sk, sv = op_signature(plain['plan']), op_signature(keep['plan']), op_signature(vox['plan'])
    assert sig == parent_ops, 'the mask=None plan differs from the plan of the parent commit'
    assert sk[0][0] == hip.OP_DDIM_BLEND and sk[1:] == sig
    assert sv[0][0] == hip.OP_DDIM_BLEND_VOX == 28 and sv[1:] == sig and all(s[0] != 28 for s in sig + sk)
    assert plain['plan'] is not keep['plan'] and keep['plan'] is not vox['plan']
    for bad in (vmask.expand(4, 3, 16, 16, 16), vmask[:3], vmask * 0.5):
        with pytest.raises(ValueError):
            den.sample(*a, x0=x0, mask=bad, keep_noise=table)


@pytest.mark.parametrize('use_graph', [False, True])
def test_plms_complete_tiny_vs_reference_golden(dev, use_graph):
    """the voxel mask under PLMS against the reference's PLMSSampler.sample(mask=z_mask, x0=) through the adapter: the blend runs once
    per iteration, in front of the first evaluation"""
    from echoscene_amd import hip
    g = load_golden('plms_complete_tiny')
    x0, vmask, table = _complete_inputs(g)
    den = _shape(dev, sampler='plms')
    z = den.sample(g['uc_s'], g['triples'], synth.shape_noise(seed=7), use_graph=use_graph, x0=x0, mask=vmask, keep_noise=table)
    e = _rel(z, g['z_final'])
    print('plms complete tiny (4 iterations, voxel mask): latent vs fp32 reference golden: rel err %.3e' % e)
    assert e < 2e-2
    st = den._plan_for(g['uc_s'], g['triples'], None, keep='vox')
    kinds = [s[0] for s in op_signature(st['first_plan'])]
    assert kinds.count(hip.OP_DDIM_BLEND_VOX) == 1 and kinds[0] == hip.OP_DDIM_BLEND_VOX
    assert [s[0] for s in op_signature(st['plan'])].count(hip.OP_DDIM_BLEND_VOX) == 1


def test_complete_shards_equal_unsharded_bitwise(dev):
    """the voxel loop sharded over 2 emulated ranks (one GPU, simulated all-gather, deterministic mode) == the unsharded run, bit for
    bit: each rank takes rows lo:hi of the mask like the other inputs (style of test_keep_shards_equal_unsharded_bitwise)"""
    g = load_golden('ddim_complete_tiny')
    x0, vmask, table = _complete_inputs(g)
    uc, triples, noise1, world, nst = g['uc_s'], g['triples'], synth.shape_noise(seed=7), 2, 4
    z_ref = _shape(dev, deterministic=True).sample(uc, triples, noise1, n_steps=nst, x0=x0, mask=vmask, keep_noise=table)
    shards = [_shape(dev, rank=r, world=world, deterministic=True) for r in range(world)]
    for sh in shards:
        st = sh._plan_for(uc, triples, None, keep='vox')
        assert tuple(st['mask'].shape) == (st['hi'] - st['lo'], 4096)
        world_, sh.world = sh.world, 1               # (fill this rank's rows from the given table: no collective draw)
        sh._fill_keep(st, x0, vmask, table)
        sh.world = world_
        assert torch.equal(st['mask'].cpu(), vmask.reshape(4, -1)[st['lo']:st['hi']])
        st['x'].copy_(noise1.to(dev).expand(st['hi'] - st['lo'], 3, 16, 16, 16))
        sh._cur, sh._use_graph = st, True
    for i in range(nst):
        codes = torch.cat([sh.codes_local(i)[:sh._cur['hi'] - sh._cur['lo']].clone() for sh in shards], 0)
        for sh in shards:
            sh.step(i, codes)
    z = torch.cat([sh.latents_local() for sh in shards], 0)
    assert torch.equal(z, z_ref), 'max abs diff %.3e' % (z - z_ref).abs().max().item()
    assert not torch.equal(z_ref, _shape(dev, deterministic=True).sample(uc, triples, noise1, n_steps=nst))


def test_complete_model_file_replays_the_python_run(dev, tmp_path):
    """save_model(keep='vox') -> es_model_load -> the regions "x0", "mask" (O * V floats) and "keep_noise" filled through ctypes ->
    es_shape_sample == ShapeDenoiser.sample, bit for bit; sampler='plms' keeps raising"""
    from echoscene_amd import hip
    from echoscene_amd.plan import Builder
    L = hip.lib()
    g = load_golden('ddim_complete_tiny')
    x0, vmask, table = _complete_inputs(g)
    den = _shape(dev)
    noise1 = synth.shape_noise(seed=7)
    ref = den.sample(g['uc_s'], g['triples'], noise1, x0=x0, mask=vmask, keep_noise=table)
    path = str(tmp_path / 'complete.esm')
    den.save_model(path, g['uc_s'], g['triples'], keep='vox')
    # (the file holds the inputs of the last run; another process would find them stale: fill every one of them)
    m = L.es_model_load(path.encode())
    assert m, L.es_last_error()
    try:
        def dcopy(dst, src, nbytes):               # device-to-device copy through the library (raw pointers: ES_OP_COPY)
            bb = Builder(dev)
            bb.copy(dst, src, nbytes)
            bb.finish().run()
            torch.cuda.synchronize()
        srcs = {b'x0': x0.to(dev).contiguous(), b'mask': vmask.reshape(4, -1).to(dev).contiguous(),
                b'keep_noise': table.reshape(4, -1).to(dev).contiguous()}
        for name, t in srcs.items():
            ptr, nb = C.c_void_p(), C.c_size_t()
            hip.check(L.es_model_region(C.c_void_p(m), name, C.byref(ptr), C.byref(nb)), 'es_model_region')
            assert nb.value == t.numel() * 4, (name, nb.value)
            # poison first: the run below may only see what is copied in now
            junk = torch.full((t.numel(),), float('nan'), device=dev)
            dcopy(ptr.value, junk.data_ptr(), nb.value)
            dcopy(ptr.value, t.data_ptr(), nb.value)
        assert srcs[b'mask'].numel() == 4 * 4096
        zT = noise1.to(dev).float().expand(4, 3, 16, 16, 16).contiguous()
        out = torch.full((4, 3, 16, 16, 16), float('nan'), device=dev)
        hip.check(L.es_shape_sample(C.c_void_p(m), C.c_void_p(zT.data_ptr()), 4, C.c_void_p(out.data_ptr()), hip.current_stream()),
                  'es_shape_sample')
        torch.cuda.synchronize()
        assert torch.equal(out, ref), 'max abs diff %.3e' % (out - ref).abs().max().item()
    finally:
        L.es_model_free(C.c_void_p(m))
    with pytest.raises(NotImplementedError):
        _shape(dev, sampler='plms').save_model(str(tmp_path / 'plms.esm'), g['uc_s'], g['triples'], keep='vox')


# ------------------------------------------------------------------------------------------------ the public interface
def test_sgdiff_complete_shapes_vs_composed_reference_golden():
    """sample_box_and_shape(complete_nodes=, complete_sdfs=, complete_ranges=, keep_nodes=, ...) against scene_complete_tiny (the
    reference's scene call with rel2shape composed from encode_no_quant -> get_partial_shape -> DDIMSampler.sample(mask, x0) ->
    decode_no_quant), with the bars of test_sgdiff_keep_shapes_vs_composed_reference_golden: boxes 1e-4, latents 2e-2, SDF samples
    outside 2e-2 of the scale at most 10 % at this object count, median 2e-3; kept rows are the caller's SDFs bit for bit.
    complete_masks=latent_range_mask(ranges) gives the same bits; an editing call takes the keywords; PLMS, a step count and kept
    boxes combine; without the keywords the call still meets scene_e2e_tiny."""
    from echoscene_amd.postprocess import latent_range_mask
    g = load_golden('scene_complete_tiny')
    objs, triples = g['objs'], g['triples']
    O = objs.shape[0]
    tf, rf = synth.synthetic_features(O, triples.shape[0], seed=9)
    comp, keep = [int(v) for v in g['complete']], [int(v) for v in g['keep']]
    cs, ks, qs = [int(v) for v in g['seeds']]
    ranges = [dict(x=(float(r[0]), float(r[1])), y=(float(r[2]), float(r[3])), z=(float(r[4]), float(r[5]))) for r in g['complete_ranges'].numpy()]
    csdfs, ksdfs = synth.ellipsoid_sdfs(len(comp), seed=cs), synth.ellipsoid_sdfs(len(keep), seed=ks)
    table = torch.stack([_rnd((O, 3, 16, 16, 16), qs + k) for k in range(4)])
    m = _build_sgdiff('echoscene')
    a = (objs.cuda(), triples.cuda(), tf.cuda(), rf.cuda())
    kw = dict(layout_noise=synth.layout_noise(O, 8, 100, seed=7), shape_noise=synth.shape_noise(seed=7))
    ckw = dict(complete_nodes=comp, complete_sdfs=csdfs, keep_nodes=keep, keep_sdfs=ksdfs, keep_noise=table)
    d = m.sample_box_and_shape(*a, gen_shape=True, complete_ranges=ranges, **ckw, **kw)
    for k in ('sizes', 'translations', 'angles'):
        assert _rel(d[k], g[k]) < 1e-4, k
    assert tuple(d['shapes'].shape) == (O, 1, 64, 64, 64)
    assert torch.equal(d['shapes'][keep].cpu(), ksdfs), 'kept rows are the caller\'s SDFs, bit for bit'
    S = m.diff.ShapeDiff
    ez = _rel(S.gen_z, g['z'])
    ex = _rel(S._encoder().encode_no_quant(torch.cat([csdfs, ksdfs])), g['x0_rows'])
    print('scene complete: encoded SDFs rel err %.2e, latents after 4 masked DDIM steps rel err %.2e' % (ex, ez))
    assert ex < 2e-2 and ez < 2e-2
    assert torch.equal(latent_range_mask(ranges, (16, 16, 16), 'cuda').cpu(), g['z_mask'].float())
    gen = [i for i in range(O) if i not in keep]              # the completed rows are decoded like the generated ones: no paste-back
    got, ref = d['shapes'][gen][:, :, ::4, ::4, ::4].cpu(), g['shapes'][gen]
    scale = ref.abs().max().item()
    bad = ((got - ref).abs() > 2e-2 * scale).float().mean().item()
    med = (got - ref).abs().median().item() / scale
    print('scene complete: decoded SDFs vs reference: %.3f%% of samples outside 2e-2, median rel err %.2e' % (100 * bad, med))
    assert bad < (0.03 if len(gen) >= 8 else 0.10) and med < 2e-3
    assert not torch.equal(d['shapes'][comp].cpu(), csdfs)
    # the voxel plan ran, once, for both families
    vox = [k for k in S._denoiser(0.0)._plans if 'keepvox' in k]
    assert len(vox) == 1 and not [k for k in S._denoiser(0.0)._plans if 'keep' in k]
    # masks in latent space instead of ranges: the same bits
    d2 = m.sample_box_and_shape(*a, gen_shape=True, complete_masks=latent_range_mask(ranges, (16, 16, 16), 'cuda'), **ckw, **kw)
    assert all(torch.equal(d2[k], d[k]) for k in ('shapes', 'sizes', 'translations', 'angles'))
    # duplicates / out-of-range entries: keep_selection's convention
    d3 = m.sample_box_and_shape(*a, gen_shape=True, complete_nodes=comp + [comp[0], 99], keep_nodes=keep, keep_sdfs=ksdfs,
                                keep_noise=table, complete_sdfs=torch.cat([csdfs, csdfs[:1] * 0, csdfs[:1] * 0]),
                                complete_ranges=ranges + [ranges[1], ranges[0]], **kw)
    assert torch.equal(d3['shapes'], d['shapes'])
    # only completed nodes (no keep_nodes): the voxel plan again; the completed rows differ from a plain generation
    d4 = m.sample_box_and_shape(*a, gen_shape=True, complete_nodes=comp, complete_sdfs=csdfs, complete_ranges=ranges, keep_noise=table, **kw)
    assert torch.isfinite(d4['shapes']).all() and not torch.equal(d4['shapes'][keep].cpu(), ksdfs)
    # an editing call takes the keywords
    np.random.seed(5)
    k5, d5 = m.sample_boxes_and_shape_with_changes(*a, *a, [1], gen_shape=True, complete_ranges=ranges, **ckw, **kw)
    assert torch.equal(d5['shapes'][keep].cpu(), ksdfs) and k5.flatten().tolist() == [1, 0] + [1] * (O - 2)
    # PLMS, a step count and kept boxes combine with it
    boxes = torch.cat([d['sizes'], d['translations'], d['angles']], 1)[[2, 5]].clone()
    d6 = m.sample_box_and_shape(*a, gen_shape=True, complete_ranges=ranges, shape_sampler='plms', shape_steps=4, keep_box_nodes=[2, 5],
                                keep_boxes=boxes, **ckw, **kw)
    assert torch.equal(d6['shapes'][keep].cpu(), ksdfs) and torch.isfinite(d6['shapes']).all()
    assert torch.equal(torch.cat([d6['sizes'], d6['translations'], d6['angles']], 1)[[2, 5]], boxes)
    # without the keywords: the call of scene_e2e_tiny
    g0 = load_golden('scene_e2e_tiny')
    d0 = m.sample_box_and_shape(*a, gen_shape=True, **kw)
    for k in ('sizes', 'translations', 'angles'):
        assert _rel(d0[k], g0['echoscene_' + k]) < 1e-4, k
    got, ref = d0['shapes'][:, :, ::4, ::4, ::4].cpu(), g0['echoscene_shapes']
    scale = ref.abs().max().item()
    assert ((got - ref).abs() > 2e-2 * scale).float().mean().item() < 0.03
