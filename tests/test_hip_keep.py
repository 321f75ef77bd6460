"""GPU tests of shape-preserving sampling: the VQ-VAE encoder (``VQVAE.encode_no_quant``), its two new conv paths, and the masked
DDIM loop (``DDIMSampler.sample(mask=, x0=)``), against goldens made by the reference itself (tests/golden/make_golden_keep.py).
Bars: the fp16-operand route's 2e-2 relative to the tensor scale (as test_vqvae_decode_vs_reference_golden and
test_ddim_loop_with_eta_vs_reference_golden); the stand-alone conv tests follow test_conv_mfma / test_conv_fp32_operand_route."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden
from echoscene_amd import synth, config as escfg

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda')


def _rel(a, b):
    a, b = a.detach().cpu().float(), b.detach().cpu().float()
    assert a.shape == b.shape, (a.shape, b.shape)
    assert torch.isfinite(a).all()
    return ((a - b).abs().max() / b.abs().max().clamp(min=1e-6)).item()


def _rnd(shape, seed, scale=1.0):
    return torch.from_numpy((np.random.RandomState(seed).standard_normal(shape) * scale).astype(np.float32))


def _cl(x):          # NCDHW -> [O*V, C]
    return x.permute(0, 2, 3, 4, 1).reshape(-1, x.shape[1]).contiguous()


def _ncdhw(y, O, D, H, W):
    return y.reshape(O, D, H, W, -1).permute(0, 4, 1, 2, 3).contiguous()


# ------------------------------------------------------------------------------------------------ the two new conv paths
@pytest.mark.parametrize('O,Cin,N,dims', [(3, 64, 48, (4, 4, 4)), (1, 32, 32, (8, 8, 8)), (5, 64, 64, (2, 4, 8))])
def test_conv_down_p01_vs_torch(dev, O, Cin, N, dims):
    """ES_CONV_DOWN_DHW_P01 (the VQ-VAE encoder's Downsample) against F.conv3d(F.pad(x, (0,1,0,1,0,1)), w, stride=2): the f16 route on
    fp16-rounded operands at test_conv_mfma's 1e-4, the fp32-operand route on unrounded operands at test_conv_fp32_operand_route's
    1e-5; the far-face voxels (last output index of each axis: the only ones that read padding) are also checked on their own, and
    the other stride-2 conv (pad 1 on both faces) must NOT match."""
    from echoscene_amd import hip
    from echoscene_amd.plan import Builder
    from echoscene_amd.plan_vol import PackedConv, PackedConv32
    D, H, W = dims
    x = _rnd((O, Cin, 2 * D, 2 * H, 2 * W), 1)
    wt = _rnd((N, Cin, 3, 3, 3), 2) / np.sqrt(Cin * 27)
    bias = _rnd((N,), 3)
    xh, wh = x.half().float(), wt.half().float()
    ref16 = F.conv3d(F.pad(xh, (0, 1, 0, 1, 0, 1)), wh, bias, stride=2)
    ref32 = F.conv3d(F.pad(x, (0, 1, 0, 1, 0, 1)), wt, bias, stride=2)
    b = Builder(dev)
    out = b.buf(O * D * H * W, N, zero=True)
    b.conv(b.dev(_cl(xh), torch.float16), PackedConv(wh, bias, dev), O, dims, mode=hip.CONV_DOWN_DHW_P01, out_f32=out)
    b.finish().run()
    b2 = Builder(dev)
    b2.fp32 = True
    out32 = b2.buf(O * D * H * W, N, zero=True)
    b2.conv(b2.dev(_cl(x)), PackedConv32(wt, bias, dev), O, dims, mode=hip.CONV_DOWN_DHW_P01, out_f32=out32)
    b2.finish().run()
    torch.cuda.synchronize()
    got, got32 = _ncdhw(out.cpu(), O, D, H, W), _ncdhw(out32.cpu(), O, D, H, W)
    e16, e32 = _rel(got, ref16), _rel(got32, ref32)
    far = [(slice(None), slice(None), -1), (slice(None), slice(None), slice(None), -1), (Ellipsis, -1), (slice(None), slice(None), -1, -1, -1)]
    ef = max(_rel(got[s], ref16[s]) for s in far)
    ef32 = max(_rel(got32[s], ref32[s]) for s in far)
    print('conv DOWN_DHW_P01 O=%d %d->%d %s: f16 route %.2e (far faces %.2e), fp32 route %.2e (far faces %.2e)' % (O, Cin, N, dims, e16, ef, e32, ef32))
    assert e16 < 1e-4 and ef < 1e-4
    assert e32 < 1e-5 and ef32 < 1e-5
    assert _rel(got, F.conv3d(xh, wh, bias, stride=2, padding=1)) > 1e-2


@pytest.mark.parametrize('O,N,dims', [(3, 32, (8, 8, 16)), (1, 64, (64, 64, 64)), (5, 16, (4, 12, 32)), (2, 128, (4, 4, 16))])
def test_conv_c1_vs_torch(dev, O, N, dims):
    """es_conv_c1_f32 (the encoder's conv_in: one input channel, fp32 in, fp32 FMA) against F.conv3d(x, w, padding=1) in fp32 torch.
    Bar 1e-5 of the tensor scale, the bar of the fp32-operand conv route: a 27-term fp32 sum in another order differs by a few
    2^-24 of sum |x w| (measured values are printed)."""
    from echoscene_amd.plan import Builder
    D, H, W = dims
    x = _rnd((O, 1, D, H, W), 11)
    wt = _rnd((N, 1, 3, 3, 3), 12) / np.sqrt(27)
    bias = _rnd((N,), 13)
    ref = F.conv3d(x, wt, bias, padding=1)
    b = Builder(dev)
    out = b.buf(O * D * H * W, N, zero=True)
    b.conv_c1(b.dev(x), b.dev(wt.flatten(1)), b.dev(bias), O, dims, out)
    b.finish().run()
    torch.cuda.synchronize()
    got = _ncdhw(out.cpu(), O, D, H, W)
    e = _rel(got, ref)
    faces = [got[:, :, 0], got[:, :, -1], got[:, :, :, 0], got[:, :, :, -1], got[..., 0], got[..., -1]]
    rfaces = [ref[:, :, 0], ref[:, :, -1], ref[:, :, :, 0], ref[:, :, :, -1], ref[..., 0], ref[..., -1]]
    ef = max(_rel(a, r) for a, r in zip(faces, rfaces))
    print('conv_c1 O=%d 1->%d %s: rel err %.2e (boundary faces %.2e)' % (O, N, dims, e, ef))
    assert e < 1e-5 and ef < 1e-5


# ------------------------------------------------------------------------------------------------ the encoder
@pytest.mark.parametrize('tag', ['tiny', 'full'])
def test_vqvae_encode_vs_reference_golden(tag):
    from echoscene_amd.model.vqvae import VQVAE
    from echoscene_amd.samplers import VQEncoder
    g = load_golden('vqvae_enc_' + tag)
    ch, ne, B, seed = [int(v) for v in g['cfg']]
    c = escfg.vqvae_conf(ch).model.params
    vq = VQVAE(dict(c.ddconfig), ne, c.embed_dim)
    synth.seeded_fill_(vq, prefix='vqvae_%s.' % tag)
    enc = VQEncoder(vq, torch.device('cuda'))
    sdf = synth.ellipsoid_sdfs(B, seed=seed)
    z = enc.encode_no_quant(sdf)
    assert tuple(z.shape) == (B, 3, 16, 16, 16)
    st = next(iter(enc._plans.values()))
    # the activations behind the two new kernels first: a failure says WHICH of them is wrong
    for name, key in (('conv_in', 'conv_in'), ('down.0', 'down0'), ('down.1', 'down1')):
        v = st['plan'].tags[name]
        n = g[key + '_far'].shape[-1]
        h = _ncdhw(v.t.cpu(), B, n, n, n)
        sub = h[:, :, ::8, ::8, ::8] if key == 'conv_in' else h[:, :, ::4, ::4, ::4]
        e1, e2 = _rel(sub, g[key + '_sub']), _rel(h[:, :, -1, -1, :], g[key + '_far'])
        ea = abs(h.double().abs().sum().item() - g[key + '_abs'].item()) / g[key + '_abs'].item()
        print('vqvae %s encode, %s: rel err %.3e (far corner line %.3e, abs-sum %.3e)' % (tag, name, e1, e2, ea))
        assert e1 < 2e-2 and e2 < 2e-2 and ea < 2e-2, name
    e = _rel(z, g['z'])
    print('vqvae %s encode: fp16-MFMA latent vs fp32 reference golden: rel err %.3e' % (tag, e))
    assert e < 2e-2
    assert st['plan'].poison_scratch() > 0                 # scratch claim of the encode plan: NaN-poisoned, same bits
    assert torch.equal(enc.encode_no_quant(sdf), z)
    # chunking: objects are independent
    if B > 1:
        enc1 = VQEncoder(vq, torch.device('cuda'), chunk=1)
        assert _rel(enc1.encode_no_quant(sdf), g['z']) < 2e-2


# ------------------------------------------------------------------------------------------------ the masked loop
def _shape(dev, S=4, **kw):
    from echoscene_amd.model.unet import DiffusionUNet
    from echoscene_amd.samplers import ShapeDenoiser
    p = escfg.shape_unet_params(32)
    p['context_dim'] = 64
    df = DiffusionUNet(p)
    synth.seeded_fill_(df, prefix='unet3d_tiny.')
    return ShapeDenoiser(df, escfg.shape_df_conf().model.params, ddim_steps=S, device=dev, **kw)


def _keep_inputs(g, O=4):
    xs, qs = [int(v) for v in g['seeds']]
    x0 = _rnd((O, 3, 16, 16, 16), xs, 0.6)
    table = torch.stack([_rnd((O, 3, 16, 16, 16), qs + k) for k in range(4)])
    mask = torch.zeros(O)
    mask[g['keep'].long()] = 1.0
    return x0, mask, table


def op_signature(plan):
    """(kind, sizes) of every op of a plan: what 'op for op the same plan' means"""
    from echoscene_amd import hip
    sig = []
    for op in plan._arr:
        k, u = op.kind, op.u
        if k == hip.OP_LINEAR:
            s = (u.linear.M, u.linear.K, u.linear.N, u.linear.nseg, u.linear.kb_per_slice)
        elif k in (hip.OP_CONV, hip.OP_CONV_F32):
            c = u.conv
            s = (c.O, c.D, c.H, c.W, c.Cin, c.N, c.taps, c.mode, c.Cin2, c.splitk, c.out_ld, c.epilogue)
        elif k == hip.OP_GN:
            s = (u.gn.O, u.gn.V, u.gn.C1, u.gn.C2, u.gn.groups, u.gn.silu)
        elif k == hip.OP_LN:
            s = (u.ln.M, u.ln.C)
        elif k in (hip.OP_ATTN, hip.OP_ATTN_F32):
            s = (u.attn.B, u.attn.Ntok, u.attn.heads, u.attn.dhead)
        elif k in (hip.OP_DDPM, hip.OP_DDIM):
            s = (u.update.n, u.update.coef_stride, u.update.inc_step)
        elif k == hip.OP_ROWSEL:
            s = (u.rowsel.rows, u.rowsel.n)
        elif k == hip.OP_COPY:
            s = (int(u.copy.bytes), u.copy.rows)
        elif k == hip.OP_TO_CL:
            s = (u.tocl.O, u.tocl.C, u.tocl.V, u.tocl.Cpad)
        elif k == hip.OP_STEM:
            s = (u.stem.O, u.stem.Cin)
        elif k == hip.OP_GEGLU:
            s = (u.geglu.M, u.geglu.C4)
        else:
            s = ()
        sig.append([int(k), int(op.lane)] + [int(v) for v in s])
    return sig


@pytest.mark.parametrize('use_graph', [False, True])
def test_ddim_keep_tiny_vs_reference_golden(dev, use_graph):
    """ShapeDenoiser.sample(x0, mask, keep_noise) against the reference's DDIMSampler.sample(mask=, x0=) with q_sample's draws
    injected; then: the blended latent the denoiser sees at the first step is the reference's bit for bit on the kept rows; mask=None
    afterwards reproduces ddim_tiny; an all-zero mask is bit-equal to the unmasked run; the mask=None plan is, op for op, the plan of
    the commit before this feature (tests/golden/shape_plan_ops_tiny.json: recorded there with op_signature() above)."""
    g = load_golden('ddim_keep_tiny')
    x0, mask, table = _keep_inputs(g)
    den = _shape(dev)
    noise1 = synth.shape_noise(seed=7)
    z = den.sample(g['uc_s'], g['triples'], noise1, use_graph=use_graph, x0=x0, mask=mask, keep_noise=table)
    e = _rel(z, g['z_final'])
    print('ddim keep tiny (4 steps, nodes %s kept): latent vs fp32 reference golden: rel err %.3e' % (g['keep'].tolist(), e))
    assert e < 2e-2
    z2 = den.sample(g['uc_s'], g['triples'], noise1, use_graph=use_graph, x0=x0, mask=mask, keep_noise=table)
    assert torch.equal(z, z2)
    st = den._plan_for(g['uc_s'], g['triples'], None, keep=True)
    assert st['plan'].poison_scratch() > 0
    assert torch.equal(den.sample(g['uc_s'], g['triples'], noise1, use_graph=use_graph, x0=x0, mask=mask, keep_noise=table), z)
    # the blend alone: step 0 of the loop up to (not including) the denoiser -> the reference's blended img
    from echoscene_amd.plan import Builder
    b = Builder(dev)
    x = b.dev(noise1.expand(4, 3, 16, 16, 16))
    step = b.buf(1, dtype=torch.int32, zero=True)
    b.blend(x, b.dev(x0), b.dev(mask), b.dev(table.reshape(4, -1)), den.keep_tab, step)
    plan = b.finish()
    plan.run()
    torch.cuda.synchronize()
    assert torch.equal(x.cpu(), g['img_first']), 'q_sample of the kept rows, the others untouched: bit for bit'
    step.fill_(3)
    x.copy_(g['img_last'].to(dev))
    x[mask.bool()] = 7.0
    plan.run()
    torch.cuda.synchronize()
    assert torch.equal(x.cpu(), g['img_last'])
    # mask=None: the old loop, the old plan
    z0 = den.sample(g['uc_s'], g['triples'], noise1, use_graph=use_graph)
    gd = load_golden('ddim_tiny')
    assert _rel(z0, gd['z_final']) < 2e-2
    zz = den.sample(g['uc_s'], g['triples'], noise1, use_graph=use_graph, x0=x0, mask=torch.zeros(4), keep_noise=table)
    assert torch.equal(zz, z0), 'an all-zero mask: the blend touches nothing'
    plain = den._plan_for(g['uc_s'], g['triples'], None)
    keep = den._plan_for(g['uc_s'], g['triples'], None, keep=True)
    with open(os.path.join(HERE, 'golden', 'shape_plan_ops_tiny.json')) as f:
        parent_ops = json.load(f)
    sig = op_signature(plain['plan'])
    assert sig == parent_ops, 'the mask=None plan differs from the plan of the parent commit'
    from echoscene_amd import hip
    sk = op_signature(keep['plan'])
    assert sk[0][0] == hip.OP_DDIM_BLEND and sk[1:] == sig and all(s[0] != hip.OP_DDIM_BLEND for s in sig)
    with pytest.raises(ValueError):
        den.sample(g['uc_s'], g['triples'], noise1, x0=x0)
    with pytest.raises(ValueError):
        den.sample(g['uc_s'], g['triples'], noise1, x0=x0, mask=torch.tensor([0.5, 0, 1, 1]))


def test_keep_shards_equal_unsharded_bitwise(dev):
    """The masked loop sharded over 2 emulated ranks (one GPU, simulated all-gather, deterministic mode) == the unsharded run, bit for
    bit: the blend is per object, each rank blends its own rows (style of test_object_shards_equal_unsharded_bitwise)."""
    g = load_golden('ddim_keep_tiny')
    x0, mask, table = _keep_inputs(g)
    uc, triples, noise1, world, nst = g['uc_s'], g['triples'], synth.shape_noise(seed=7), 2, 4
    z_ref = _shape(dev, deterministic=True).sample(uc, triples, noise1, n_steps=nst, x0=x0, mask=mask, keep_noise=table)
    shards = [_shape(dev, rank=r, world=world, deterministic=True) for r in range(world)]
    for sh in shards:
        st = sh._plan_for(uc, triples, None, keep=True)
        world_, sh.world = sh.world, 1               # (fill this rank's rows from the given table: no collective draw)
        sh._fill_keep(st, x0, mask, table)
        sh.world = world_
        st['x'].copy_(noise1.to(dev).expand(st['hi'] - st['lo'], 3, 16, 16, 16))
        sh._cur, sh._use_graph = st, True
    for i in range(nst):
        codes = torch.cat([sh.codes_local(i)[:sh._cur['hi'] - sh._cur['lo']].clone() for sh in shards], 0)
        for sh in shards:
            sh.step(i, codes)
    z = torch.cat([sh.latents_local() for sh in shards], 0)
    assert torch.equal(z, z_ref), 'max abs diff %.3e' % (z - z_ref).abs().max().item()
    assert not torch.equal(z_ref, _shape(dev, deterministic=True).sample(uc, triples, noise1, n_steps=nst))


# ------------------------------------------------------------------------------------------------ the public interface
def _build_sgdiff(typ):
    from model.SGDiff import SGDiff
    m = SGDiff(typ, escfg.tiny_diff_opt('cuda'), synth.VOCAB, replace_latent=False, with_changes=True, residual=True,
               gconv_pooling='avg', with_angles=True, clip=True, separated=False)
    synth.seeded_fill_(torch.nn.Module.state_dict(m.diff), prefix='e2e.diff.')
    if typ == 'echoscene':
        synth.seeded_fill_(m.diff.ShapeDiff.df, prefix='e2e.shape_df.')
        synth.seeded_fill_(m.diff.ShapeDiff.vqvae, prefix='e2e.vqvae.')
        m.diff.ShapeDiff.ddim_steps = 4
    m.diff.optimizer_ini()
    m.cuda()
    m.eval()
    return m


def test_sgdiff_keep_shapes_vs_composed_reference_golden():
    """sample_box_and_shape(keep_nodes=, keep_sdfs=) against scene_keep_tiny (the reference's scene call with its rel2shape composed
    from encode_no_quant -> DDIMSampler.sample(mask, x0) -> decode_no_quant); bars of test_sgdiff_api_end_to_end_vs_reference_golden
    (boxes 1e-4, SDF as a distribution) and the latents before the codebook argmin at 2e-2.  Kept rows are the caller's SDFs bit for
    bit; without the keywords the call still meets scene_e2e_tiny; an 'echolayout' model refuses the keywords."""
    g = load_golden('scene_keep_tiny')
    objs, triples = g['objs'], g['triples']
    O = objs.shape[0]
    tf, rf = synth.synthetic_features(O, triples.shape[0], seed=9)
    keep = [int(v) for v in g['keep']]
    ss, qs = [int(v) for v in g['seeds']]
    sdfs = synth.ellipsoid_sdfs(len(keep), seed=ss)
    table = torch.stack([_rnd((O, 3, 16, 16, 16), qs + k) for k in range(4)])
    m = _build_sgdiff('echoscene')
    a = (objs.cuda(), triples.cuda(), tf.cuda(), rf.cuda())
    kw = dict(layout_noise=synth.layout_noise(O, 8, 100, seed=7), shape_noise=synth.shape_noise(seed=7))
    d = m.sample_box_and_shape(*a, gen_shape=True, keep_nodes=keep, keep_sdfs=sdfs, keep_noise=table, **kw)
    for k in ('sizes', 'translations', 'angles'):
        assert _rel(d[k], g[k]) < 1e-4, k
    assert tuple(d['shapes'].shape) == (O, 1, 64, 64, 64)
    assert torch.equal(d['shapes'][keep].cpu(), sdfs), 'kept rows are the caller\'s SDFs, bit for bit'
    ez = _rel(m.diff.ShapeDiff.gen_z, g['z'])
    ex = _rel(m.diff.ShapeDiff._encoder().encode_no_quant(sdfs), g['x0_keep'])
    print('scene keep: encoded kept SDFs rel err %.2e, latents after 4 masked DDIM steps rel err %.2e' % (ex, ez))
    assert ex < 2e-2 and ez < 2e-2
    gen = [i for i in range(O) if i not in keep]
    got, ref = d['shapes'][gen][:, :, ::4, ::4, ::4].cpu(), g['shapes'][gen]
    scale = ref.abs().max().item()
    bad = ((got - ref).abs() > 2e-2 * scale).float().mean().item()
    med = (got - ref).abs().median().item() / scale
    print('scene keep: generated SDFs vs reference: %.3f%% of samples outside 2e-2, median rel err %.2e' % (100 * bad, med))
    assert bad < (0.03 if len(gen) >= 8 else 0.10) and med < 2e-3
    # duplicates / out-of-range entries: the manipulated_nodes convention
    d2 = m.sample_box_and_shape(*a, gen_shape=True, keep_nodes=keep + [keep[0], 99], keep_noise=table,
                                keep_sdfs=torch.cat([sdfs, sdfs[:1] * 0, sdfs[:1] * 0]), **kw)
    assert torch.equal(d2['shapes'], d['shapes'])
    # editing calls take the keywords too
    np.random.seed(5)
    k3, d3 = m.sample_boxes_and_shape_with_changes(*a, *a, [1], gen_shape=True, keep_nodes=keep, keep_sdfs=sdfs, keep_noise=table, **kw)
    assert torch.equal(d3['shapes'][keep].cpu(), sdfs) and k3.flatten().tolist() == [1, 0] + [1] * (O - 2)
    # without the keywords: the call of scene_e2e_tiny
    g0 = load_golden('scene_e2e_tiny')
    d0 = m.sample_box_and_shape(*a, gen_shape=True, **kw)
    for k in ('sizes', 'translations', 'angles'):
        assert _rel(d0[k], g0['echoscene_' + k]) < 1e-4, k
    got, ref = d0['shapes'][:, :, ::4, ::4, ::4].cpu(), g0['echoscene_shapes']
    scale = ref.abs().max().item()
    assert ((got - ref).abs() > 2e-2 * scale).float().mean().item() < 0.03
    with pytest.raises(ValueError):
        m.sample_box_and_shape(*a, gen_shape=True, keep_nodes=keep, **kw)
    with pytest.raises(ValueError):
        m.sample_box_and_shape(*a, gen_shape=False, keep_nodes=keep, keep_sdfs=sdfs, layout_noise=kw['layout_noise'])
    ml = _build_sgdiff('echolayout')
    with pytest.raises(ValueError):
        ml.sample_box_and_shape(*a, keep_nodes=keep, keep_sdfs=sdfs, layout_noise=kw['layout_noise'])
    with pytest.raises(ValueError):
        ml.sample_boxes_and_shape_with_changes(*a, *a, [1], keep_nodes=keep, keep_sdfs=sdfs, layout_noise=kw['layout_noise'])
