#!/usr/bin/env python
"""Golden vectors of shape completion (per-voxel keep masks in the masked shape loop), from the REFERENCE ITSELF (read-only).

    python tests/golden/make_golden_complete.py --ref <checkout of the reference> [--only NAME]

Loads make_golden.py / make_golden_keep.py / make_golden_plms.py for their helpers and stores numbers only.  Inputs that a formula
and a seed reproduce (SDFs of ellipsoids, normal draws) are NOT stored: the tests rebuild them from the same seeds.

``get_partial_shape`` lives in model/networks/diffusion_shape/diff_utils/demo_util.py, whose imports name packages of the shape
branch's parent project (``datasets.*``, ``models.*``, ``utils.*``) that do not exist in the tree: the file is imported behind empty
stand-in modules of those names (removed again afterwards), as the PLMS generator imports plms.py behind an alias.  The function
itself runs unchanged.

  partial_shape_ranges: ``get_partial_shape`` on ``synth.ellipsoid_sdfs(2, seed=85)`` with a 16^3 ``z``, for the six RANGES below:
      z_mask whole (uint8), shape_mask as packed bits, shape_part / shape_missing [::4] per axis with their abs().sum(), and the
      integer bounds read back from the two masks (-1 where a mask is empty).
  ddim_complete_tiny: ``DDIMSampler.sample(S=4, mask=z_mask, x0=)`` on the model of ddim_tiny; O = 4: node 0 range 1, node 1 all
      ones, node 2 range 2, node 3 all zero; q_sample's draws injected.
  plms_complete_tiny: the same through the PLMS adapter.
  scene_complete_tiny: the scene call of scene_keep_tiny with rel2shape composed from encode_no_quant (of the WHOLE given SDFs),
      get_partial_shape (z_mask), DDIMSampler.sample(mask, x0) and decode_no_quant.  O = 8, nodes SCENE_COMPLETE completed (ranges 2
      and 3), node SCENE_KEEP kept whole.
"""
import argparse
import importlib
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


mk = _load('make_golden_keep')
mg = mk.mg
synth, escfg, fill, rnd, save = mg.synth, mg.escfg, mg.fill, mg.rnd, mg.save

FULL = (-1.0, 1.0)
RANGES = [                                     # numbered 1..6 in the texts
    dict(x=FULL, y=(-1.0, 0.0), z=FULL),
    dict(x=(-0.3, 0.45), y=FULL, z=(-0.6, 1.0)),             # innermost axis not 4-aligned at 16^3: mixed lanes
    dict(x=(-2.0, 0.1), y=(-0.55, 3.0), z=(-0.9, 0.3)),      # clamped to [-1, 1]
    dict(x=(0.5, -0.5), y=FULL, z=FULL),                     # empty
    dict(x=FULL, y=FULL, z=FULL),                            # the full cube
    dict(x=(0.2, 0.3), y=(0.2, 0.3), z=(0.2, 0.3)),          # one latent voxel
]
SDF_SEED = 85
X0_SEED, QNOISE_SEED = 61, 950                 # the inputs of ddim_keep_tiny
SCENE_COMPLETE, SCENE_RANGES, SCENE_KEEP = [1, 4], [1, 2], [6]       # (SCENE_RANGES: indices into RANGES)
SCENE_SDF_SEED, SCENE_KEEP_SDF_SEED, SCENE_QNOISE_SEED = 87, 88, 980


def partial_shape_fn():
    """the reference's get_partial_shape, importable"""
    names = ('datasets', 'datasets.base_dataset', 'datasets.dataloader', 'models', 'models.base_model', 'utils', 'utils.util')
    saved = {n: sys.modules.get(n) for n in names}
    for n in names:
        m = types.ModuleType(n)
        m.__path__ = []
        sys.modules[n] = m
    for n, attrs in (('datasets.base_dataset', ('CreateDataset',)), ('datasets.dataloader', ('CreateDataLoader', 'get_data_generator')),
                     ('models.base_model', ('create_model',)), ('utils.util', ('seed_everything',))):
        for a in attrs:
            setattr(sys.modules[n], a, None)
    try:
        mod = importlib.import_module('model.networks.diffusion_shape.diff_utils.demo_util')
    finally:
        for n, m in saved.items():
            if m is None:
                sys.modules.pop(n, None)
            else:
                sys.modules[n] = m
    return mod.get_partial_shape


def ranges_array(ranges=RANGES):
    return np.array([[r['x'][0], r['x'][1], r['y'][0], r['y'][1], r['z'][0], r['z'][1]] for r in ranges], np.float64)


def _bounds_of(mask):
    """(st, ed) per axis of a box-shaped 0/1 mask [D, H, W]; -1 everywhere when it is empty"""
    m = np.asarray(mask) != 0
    if not m.any():
        return [-1] * 6
    out = []
    for ax in range(3):
        hit = np.nonzero(m.any(axis=tuple(a for a in range(3) if a != ax)))[0]
        out += [int(hit[0]), int(hit[-1]) + 1]
    return out


def z_masks(gps, ranges, zdims=(16, 16, 16)):
    """z_mask [len(ranges), 1, *zdims] of the reference, one call per range (get_partial_shape takes one xyz_dict per batch)"""
    shape = torch.zeros(1, 1, *[4 * d for d in zdims])
    z = torch.zeros(1, 3, *zdims)
    return torch.cat([gps(shape, r, z=z)['z_mask'] for r in ranges], 0)


def case_partial_shape_ranges():
    gps = partial_shape_fn()
    sdf = synth.ellipsoid_sdfs(2, seed=SDF_SEED)
    z = torch.zeros(2, 3, 16, 16, 16)
    out = dict(ranges=ranges_array(), sdf_seed=np.array([SDF_SEED]))
    zm, sm, b16, b64, part, miss, pa, ma = [], [], [], [], [], [], [], []
    for r in RANGES:
        ret = gps(sdf, r, z=z)
        assert torch.equal(ret['z_mask'][0], ret['z_mask'][1]) and torch.equal(ret['shape_mask'][0], ret['shape_mask'][1])
        zm.append(ret['z_mask'][0, 0].numpy().astype(np.uint8))
        sm.append(np.packbits(ret['shape_mask'][0, 0].numpy().reshape(-1)))
        b16.append(_bounds_of(ret['z_mask'][0, 0]))
        b64.append(_bounds_of(ret['shape_mask'][0, 0]))
        part.append(ret['shape_part'][:, :, ::4, ::4, ::4])
        miss.append(ret['shape_missing'][:, :, ::4, ::4, ::4])
        pa.append(float(ret['shape_part'].double().abs().sum()))
        ma.append(float(ret['shape_missing'].double().abs().sum()))
        print(r, b16[-1], b64[-1], int(ret['z_mask'][0].sum()), int(ret['shape_mask'][0].sum()))
    save('partial_shape_ranges', z_mask=np.stack(zm), shape_mask_bits=np.stack(sm), bounds16=np.array(b16), bounds64=np.array(b64),
         shape_part_sub=torch.stack(part), shape_missing_sub=torch.stack(miss), shape_part_abs=np.array(pa),
         shape_missing_abs=np.array(ma), **out)


def _complete_inputs(gps, O=4):
    x0 = rnd((O, 3, 16, 16, 16), X0_SEED, 0.6)
    table = torch.stack([rnd((O, 3, 16, 16, 16), QNOISE_SEED + k) for k in range(4)])
    mask = torch.zeros(O, 1, 16, 16, 16)
    mask[0:1] = z_masks(gps, [RANGES[0]])
    mask[1] = 1.0
    mask[2:3] = z_masks(gps, [RANGES[1]])
    return x0, table, mask


def case_ddim_complete_tiny():
    gps = partial_shape_fn()
    net = mg._unet3d(32, 64)
    fill(net, 'unet3d_tiny.')
    shim, EchoToShape, DDIMSampler = mk._keep_sampler(net)
    O = 4
    objs, triples = synth.synthetic_graph(O, seed=6)
    uc, c = rnd((O, 1, 64), 52), rnd((O, 1, 64), 53)
    noise1 = synth.shape_noise(seed=7)
    x0, table, mask = _complete_inputs(gps, O)
    n = mk._inject_q_noise(shim, lambda xs, t, noise: EchoToShape.q_sample(shim, xs, t, noise=noise), table)
    sampler = DDIMSampler(shim)
    seen = []
    p_orig = sampler.p_sample_ddim

    def p_sample(x, *a, **k):
        seen.append(x.clone())
        return p_orig(x, *a, **k)
    sampler.p_sample_ddim = p_sample
    with torch.no_grad():
        z, _ = sampler.sample(S=4, batch_size=O, shape=(3, 16, 16, 16), conditioning=c, x_T=noise1.repeat(O, 1, 1, 1, 1),
                              verbose=False, unconditional_guidance_scale=3., unconditional_conditioning=uc, triplet=triples,
                              eta=0.0, mask=mask, x0=x0)
    assert n['i'] == 4 and len(seen) == 4
    save('ddim_complete_tiny', uc_s=uc, triples=triples, seeds=np.array([X0_SEED, QNOISE_SEED]), z_mask=mask.numpy().astype(np.uint8),
         z_final=z, img_first=seen[0], img_last=seen[-1])


def case_plms_complete_tiny():
    mp = _load('make_golden_plms')
    gps = partial_shape_fn()
    PLMSSampler = mp.plms_sampler_class()
    shim, EchoToShape, ad, O, triples, uc, c, noise1 = mp._tiny()
    x0, table, mask = _complete_inputs(gps, O)
    n = {'i': 0}

    def q(x_start, t, noise=None):
        i = n['i']
        n['i'] += 1
        return EchoToShape.q_sample(shim, x_start, t, noise=table[i].clone())
    ad.q_sample = q
    sampler = PLMSSampler(ad)
    seen = []
    p_orig = sampler.p_sample_plms

    def p(x, *a, **k):
        seen.append(x.clone())
        return p_orig(x, *a, **k)
    sampler.p_sample_plms = p
    with torch.no_grad():
        z, _ = sampler.sample(S=4, batch_size=O, shape=(3, 16, 16, 16), conditioning=c, x_T=noise1.repeat(O, 1, 1, 1, 1),
                              verbose=False, eta=0.0, mask=mask, x0=x0)
    assert n['i'] == 4 and len(seen) == 4 and len(ad.calls) == 5
    save('plms_complete_tiny', uc_s=uc, triples=triples, seeds=np.array([X0_SEED, QNOISE_SEED]), z_mask=mask.numpy().astype(np.uint8),
         z_final=z, img_first=seen[0], img_last=seen[-1], calls=np.array(ad.calls))


def case_scene_complete_tiny():
    import tempfile
    gps = partial_shape_fn()
    tmp = tempfile.mkdtemp(prefix='golden_complete_')
    vq = mg._vqvae(32, 64)
    fill(vq, 'e2e.vqvae.')
    vq_path = os.path.join(tmp, 'vq.pth')
    torch.save(vq.state_dict(), vq_path)
    opt = escfg.tiny_diff_opt(device='cpu', logs_dir=tmp, vq_ckpt=vq_path)
    opt.misc.debug = 0
    import model.networks.diffusion_shape.echo2shape as e2s
    e2s.init_mesh_renderer = lambda **k: None
    from model.networks.diffusion_shape.samplers.ddim import DDIMSampler
    DDIMSampler.register_buffer = lambda self, name, attr: setattr(self, name, attr)
    from model.SGDiff import SGDiff
    m = SGDiff('echoscene', opt, synth.VOCAB, replace_latent=False, with_changes=True, residual=True,
               gconv_pooling='avg', with_angles=True, clip=True, separated=False)
    synth.seeded_fill_(torch.nn.Module.state_dict(m.diff), seed=0, prefix='e2e.diff.')
    S = m.diff.ShapeDiff
    fill(S.df, 'e2e.shape_df.')
    S.ddim_steps = 4
    m.eval()
    O = 8
    objs, triples = synth.synthetic_graph(O, seed=9)
    tf, rf = synth.synthetic_features(O, triples.shape[0], seed=9)
    noise = synth.layout_noise(O, 8, 100, seed=7)
    noise1 = synth.shape_noise(seed=7)
    sdfs = synth.ellipsoid_sdfs(len(SCENE_COMPLETE), seed=SCENE_SDF_SEED)
    keep_sdfs = synth.ellipsoid_sdfs(len(SCENE_KEEP), seed=SCENE_KEEP_SDF_SEED)
    table = torch.stack([rnd((O, 3, 16, 16, 16), SCENE_QNOISE_SEED + k) for k in range(4)])
    rec = {}

    def rel2shape_complete(data, ddim_eta=0.0):
        """rel2shape (echo2shape.py:484-525) with the sampler's mask / x0 arguments filled as shape_comp fills them
        (sdfusion_model.py:400-446): the whole SDF encoded, z_mask of get_partial_shape"""
        S.switch_eval()
        S.set_input(data)
        B = S.rel.shape[0]
        x0 = torch.zeros((B,) + tuple(S.z_shape))
        mask = torch.zeros(B, 1, *S.z_shape[1:])
        for k, node in enumerate(SCENE_COMPLETE):
            z = S.vqvae_module.encode_no_quant(sdfs[k:k + 1])
            ret = gps(sdfs[k:k + 1], RANGES[SCENE_RANGES[k]], z=z)
            x0[node], mask[node] = z[0], ret['z_mask'][0]
        x0[SCENE_KEEP] = S.vqvae_module.encode_no_quant(keep_sdfs)
        mask[SCENE_KEEP] = 1.0
        q_orig = S.q_sample
        n = mk._inject_q_noise(S, lambda xs, t, noise: q_orig(xs, t, noise=noise), table)
        try:
            samples, _ = DDIMSampler(S).sample(S=S.ddim_steps, batch_size=B, shape=S.z_shape, conditioning=S.rel,
                                               x_T=noise1.repeat(B, 1, 1, 1, 1), verbose=False,
                                               unconditional_guidance_scale=S.uc_scale, unconditional_conditioning=S.uc_rel,
                                               triplet=S.triples, eta=ddim_eta, mask=mask, x0=x0)
        finally:
            del S.q_sample
        assert n['i'] == 4
        rec['z'], rec['x0'], rec['mask'] = samples, x0, mask
        S.gen_df = S.vqvae_module.decode_no_quant(samples)
        return S.gen_df
    S.rel2shape = rel2shape_complete
    import model.networks.diffusion_layout.diffusion_ddpm as dd
    _orig_gen = dd.DiffusionPoint.gen_samples_sg
    calls = {'n': 0}

    def noise_fn(size, dtype, device):
        i = calls['n']
        calls['n'] += 1
        return noise[i].clone()

    def gen(self, shape, device, obj_embed, triples=None, condition=None, noise_fn_=None, clip_denoised=True,
            keep_running=False, **kw):
        return _orig_gen(self, shape, device, obj_embed, triples, condition=condition, noise_fn=noise_fn,
                         clip_denoised=clip_denoised, keep_running=keep_running)
    dd.DiffusionPoint.gen_samples_sg = gen
    try:
        with torch.no_grad():
            d = m.sample_box_and_shape(objs, triples, tf, rf, gen_shape=True)
    finally:
        dd.DiffusionPoint.gen_samples_sg = _orig_gen
    assert calls['n'] == 101, calls
    out = dict(objs=objs, triples=triples, complete=np.array(SCENE_COMPLETE), complete_ranges=ranges_array([RANGES[i] for i in SCENE_RANGES]),
               keep=np.array(SCENE_KEEP), seeds=np.array([SCENE_SDF_SEED, SCENE_KEEP_SDF_SEED, SCENE_QNOISE_SEED]),
               z=rec['z'], x0_rows=rec['x0'][SCENE_COMPLETE + SCENE_KEEP], z_mask=rec['mask'][SCENE_COMPLETE].numpy().astype(np.uint8),
               shapes=d['shapes'][:, :, ::4, ::4, ::4], shapes_abs=d['shapes'].double().abs().sum())
    for k in ('sizes', 'translations', 'angles'):
        out[k] = d[k]
    save('scene_complete_tiny', **out)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--only', default=None)
    ap.add_argument('--ref', required=True, help='checkout of the reference (read-only)')
    args = ap.parse_args()
    mg.install_reference(args.ref)
    cases = dict(partial_shape_ranges=case_partial_shape_ranges, ddim_complete_tiny=case_ddim_complete_tiny,
                 plms_complete_tiny=case_plms_complete_tiny, scene_complete_tiny=case_scene_complete_tiny)
    for name, fn in cases.items():
        if args.only in (None, name):
            fn()
