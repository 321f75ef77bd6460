#!/usr/bin/env python
"""Golden vectors of shape-preserving sampling (VQ-VAE encoder + masked DDIM), from the REFERENCE ITSELF (read-only).

    python tests/golden/make_golden_keep.py --ref <checkout of the reference> [--only NAME]

Loads make_golden.py for its helpers (reference import with stand-ins, seeded fill, save) and stores numbers only.  Inputs that a
formula and a seed reproduce (SDFs of ellipsoids, normal draws) are NOT stored: the tests rebuild them from the same seeds.

  vqvae_enc_{tiny,full}: ``VQVAE.encode_no_quant`` on ``synth.ellipsoid_sdfs(B, seed=81)``; z whole, the activation after conv_in
      ([::8] per axis: [::4] of a 64^3 x ch tensor alone would exceed the size limit of a committed file) and after each
      Downsample ([::4], and the far corner line, which [::4] never reaches), each with its abs().sum().
  ddim_keep_tiny: ``DDIMSampler.sample(S=4, mask=, x0=)`` on the model of ddim_tiny, nodes KEEP kept, q_sample's draws injected.
  scene_keep_tiny: the scene call of scene_e2e_tiny with the reference's rel2shape replaced by a composition of reference parts:
      vqvae.encode_no_quant on the kept SDFs -> DDIMSampler.sample(mask, x0) -> vqvae.decode_no_quant.
"""
import argparse
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location('make_golden', os.path.join(HERE, 'make_golden.py'))
mg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mg)
synth, escfg, fill, rnd, save = mg.synth, mg.escfg, mg.fill, mg.rnd, mg.save

SDF_SEED = 81
KEEP = [1, 3]                 # kept nodes of ddim_keep_tiny (O = 4)
X0_SEED, QNOISE_SEED = 61, 950
SCENE_KEEP = [0, 2, 5, 6]     # kept nodes of scene_keep_tiny (O = 8)
SCENE_SDF_SEED, SCENE_QNOISE_SEED = 83, 970


def case_vqvae_enc():
    for tag, ch, ne, B in (('tiny', 32, 64, 2), ('full', 64, 8192, 1)):
        vq = mg._vqvae(ch, ne)
        fill(vq, 'vqvae_%s.' % tag)
        x = synth.ellipsoid_sdfs(B, seed=SDF_SEED)
        grab = {}
        hooks = [vq.encoder.conv_in.register_forward_hook(lambda m, i, o: grab.__setitem__('conv_in', o))]
        for lvl, d in enumerate(vq.encoder.down):
            if hasattr(d, 'downsample'):
                hooks.append(d.downsample.register_forward_hook(lambda m, i, o, k='down%d' % lvl: grab.__setitem__(k, o)))
        with torch.no_grad():
            z = vq.encode_no_quant(x)
        for h in hooks:
            h.remove()
        out = dict(z=z, cfg=np.array([ch, ne, B, SDF_SEED]))
        for k, h in grab.items():
            out[k + '_sub'] = h[:, :, ::8, ::8, ::8] if k == 'conv_in' else h[:, :, ::4, ::4, ::4]
            out[k + '_far'] = h[:, :, -1, -1, :]
            out[k + '_abs'] = h.double().abs().sum()
        print(tag, 'max|z| %.3f std %.3f' % (z.abs().max(), z.std()))
        save('vqvae_enc_' + tag, **out)


def _keep_sampler(net):
    """the reference's DDIMSampler on a shim carrying the model's schedule, apply_model and q_sample (make_golden.case_ddim_tiny)"""
    from model.networks.diffusion_shape.echo2shape import EchoToShape
    from model.networks.diffusion_shape.samplers.ddim import DDIMSampler
    shim = mg._ShapeShim()
    shim.df = shim.df_module = net
    EchoToShape.register_schedule(shim, timesteps=1000, linear_start=0.00085, linear_end=0.012)
    shim.apply_model = lambda *a, **k: EchoToShape.apply_model(shim, *a, **k)
    DDIMSampler.register_buffer = lambda self, name, attr: setattr(self, name, attr)   # cuda-free
    return shim, EchoToShape, DDIMSampler


def _inject_q_noise(model, q_sample, table):
    """q_sample draws with randn_like: hand it the rows of ``table`` instead, in call order"""
    n = {'i': 0}

    def q(x_start, t, noise=None):
        i = n['i']
        n['i'] += 1
        return q_sample(x_start, t, noise=table[i].clone())
    model.q_sample = q
    return n


def case_ddim_keep_tiny():
    net = mg._unet3d(32, 64)
    fill(net, 'unet3d_tiny.')
    shim, EchoToShape, DDIMSampler = _keep_sampler(net)
    O = 4
    objs, triples = synth.synthetic_graph(O, seed=6)
    uc, c = rnd((O, 1, 64), 52), rnd((O, 1, 64), 53)
    noise1 = synth.shape_noise(seed=7)
    x0 = rnd((O, 3, 16, 16, 16), X0_SEED, 0.6)
    table = torch.stack([rnd((O, 3, 16, 16, 16), QNOISE_SEED + k) for k in range(4)])
    mask = torch.zeros(O, 1, 1, 1, 1)
    mask[KEEP] = 1.0
    n = _inject_q_noise(shim, lambda xs, t, noise: EchoToShape.q_sample(shim, xs, t, noise=noise), table)
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
    s100 = DDIMSampler(shim)
    s100.make_schedule(ddim_num_steps=100, ddim_eta=0.0, verbose=False)
    ts4, ts100 = np.asarray(sampler.ddim_timesteps), np.asarray(s100.ddim_timesteps)
    save('ddim_keep_tiny', uc_s=uc, triples=triples, keep=np.array(KEEP), seeds=np.array([X0_SEED, QNOISE_SEED]), z_final=z,
         img_first=seen[0], img_last=seen[-1], ts4=ts4, ts100=ts100,
         sac4=shim.sqrt_alphas_cumprod[ts4], s1mac4=shim.sqrt_one_minus_alphas_cumprod[ts4],
         sac100=shim.sqrt_alphas_cumprod[ts100], s1mac100=shim.sqrt_one_minus_alphas_cumprod[ts100])


def case_scene_keep_tiny():
    import tempfile
    tmp = tempfile.mkdtemp(prefix='golden_keep_')
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
    sdfs = synth.ellipsoid_sdfs(len(SCENE_KEEP), seed=SCENE_SDF_SEED)
    table = torch.stack([rnd((O, 3, 16, 16, 16), SCENE_QNOISE_SEED + k) for k in range(4)])
    rec = {}

    def rel2shape_keep(data, ddim_eta=0.0):
        """rel2shape (echo2shape.py:484-525) with the sampler's mask / x0 arguments filled from the encoded kept SDFs"""
        S.switch_eval()
        S.set_input(data)
        B = S.rel.shape[0]
        x0 = torch.zeros((B,) + tuple(S.z_shape))
        x0[SCENE_KEEP] = S.vqvae_module.encode_no_quant(sdfs)
        mask = torch.zeros(B, 1, 1, 1, 1)
        mask[SCENE_KEEP] = 1.0
        q_orig = S.q_sample
        n = _inject_q_noise(S, lambda xs, t, noise: q_orig(xs, t, noise=noise), table)
        try:
            samples, _ = DDIMSampler(S).sample(S=S.ddim_steps, batch_size=B, shape=S.z_shape, conditioning=S.rel,
                                               x_T=noise1.repeat(B, 1, 1, 1, 1), verbose=False,
                                               unconditional_guidance_scale=S.uc_scale, unconditional_conditioning=S.uc_rel,
                                               triplet=S.triples, eta=ddim_eta, mask=mask, x0=x0)
        finally:
            del S.q_sample
        assert n['i'] == 4
        rec['z'], rec['x0'] = samples, x0
        S.gen_df = S.vqvae_module.decode_no_quant(samples)
        return S.gen_df
    S.rel2shape = rel2shape_keep
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
    out = dict(objs=objs, triples=triples, keep=np.array(SCENE_KEEP), seeds=np.array([SCENE_SDF_SEED, SCENE_QNOISE_SEED]),
               z=rec['z'], x0_keep=rec['x0'][SCENE_KEEP], shapes=d['shapes'][:, :, ::4, ::4, ::4],
               shapes_abs=d['shapes'].double().abs().sum())
    for k in ('sizes', 'translations', 'angles'):
        out[k] = d[k]
    save('scene_keep_tiny', **out)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--only', default=None)
    ap.add_argument('--ref', required=True, help='checkout of the reference (read-only)')
    args = ap.parse_args()
    mg.install_reference(args.ref)
    cases = dict(vqvae_enc=case_vqvae_enc, ddim_keep_tiny=case_ddim_keep_tiny, scene_keep_tiny=case_scene_keep_tiny)
    for name, fn in cases.items():
        if args.only in (None, name):
            fn()
