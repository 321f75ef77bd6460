#!/usr/bin/env python
"""Golden vectors of PLMS shape sampling, from the REFERENCE ITSELF (read-only): its ``PLMSSampler``
(model/networks/diffusion_shape/samplers/plms.py) on the EchoScene shape model.

    python tests/golden/make_golden_plms.py --ref <checkout of the reference> [--only NAME]

Loads make_golden.py for its helpers (reference import with stand-ins, seeded fill, save) and stores numbers only.  As shipped the
reference's sampler cannot be imported or called on EchoToShape; three things make it run, none of which touches its arithmetic:
  * its import ``models.networks.diffusion_networks.ldm_diffusion_util`` names a package that does not exist in the tree: the real
    ``model.networks.diffusion_shape.ldm_diffusion_util`` is registered under that name in ``sys.modules``;
  * ``PLMSSampler.register_buffer`` moves every table to 'cuda': replaced by a plain setattr, as is done for DDIMSampler;
  * it calls ``apply_model(x, t, c)`` while ``EchoToShape.apply_model`` takes ``(x, obj_embed, triples, t, cond)``: an adapter in
    front of the model forwards ``apply_model(x, t, c)`` to ``EchoToShape.apply_model(model, x, uc, triples, t, c)`` -- the call
    DDIMSampler.p_sample_ddim makes (samplers/ddim.py:207-217).

  plms_tiny: ``PLMSSampler.sample(S)`` for S = 4 and S = 5 on the model and the inputs of ddim_tiny.  z_final whole, the timesteps the
      denoiser was called at, and per iteration the state after it ([::4] per axis) with its abs().sum().
  plms_keep_tiny: S = 4 with ``mask`` / ``x0`` as in ddim_keep_tiny (nodes [1, 3] kept, q_sample's draws injected).
  scene_plms_tiny: the scene call of scene_e2e_tiny with the reference's rel2shape replaced by a composition of reference parts:
      PLMSSampler through the adapter (S = 4) -> vqvae.decode_no_quant.
"""
import argparse
import importlib
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

KEEP = [1, 3]                 # kept nodes of plms_keep_tiny (O = 4): the inputs of ddim_keep_tiny
X0_SEED, QNOISE_SEED = 61, 950


def plms_sampler_class():
    """the reference's PLMSSampler, importable and CUDA-free"""
    real = importlib.import_module('model.networks.diffusion_shape.ldm_diffusion_util')
    import types
    for name in ('models', 'models.networks', 'models.networks.diffusion_networks'):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules['models.networks.diffusion_networks.ldm_diffusion_util'] = real
    from model.networks.diffusion_shape.samplers.plms import PLMSSampler
    PLMSSampler.register_buffer = lambda self, name, attr: setattr(self, name, attr)
    return PLMSSampler


class Adapter:
    """what PLMSSampler touches of its model, with ``apply_model(x, t, c)`` forwarded to EchoToShape's five-argument apply_model"""

    def __init__(self, model, apply5, uc, triples):
        self._m, self._apply5, self._uc, self._triples = model, apply5, uc, triples
        self.calls = []

    def __getattr__(self, name):
        return getattr(self._m, name)

    def apply_model(self, x, t, c):
        self.calls.append(int(t[0]))
        assert bool((t == t[0]).all())
        return self._apply5(x, self._uc, self._triples, t, c)


def _record_states(sampler):
    """the state after every iteration (p_sample_plms returns it first)"""
    states = []
    p_orig = sampler.p_sample_plms

    def p(*a, **k):
        outs = p_orig(*a, **k)
        states.append(outs[0].clone())
        return outs
    sampler.p_sample_plms = p
    return states


def _tiny():
    from model.networks.diffusion_shape.echo2shape import EchoToShape
    net = mg._unet3d(32, 64)
    fill(net, 'unet3d_tiny.')
    shim = mg._ShapeShim()
    shim.df = shim.df_module = net
    EchoToShape.register_schedule(shim, timesteps=1000, linear_start=0.00085, linear_end=0.012)
    O = 4
    objs, triples = synth.synthetic_graph(O, seed=6)
    uc, c = rnd((O, 1, 64), 52), rnd((O, 1, 64), 53)
    noise1 = synth.shape_noise(seed=7)
    ad = Adapter(shim, lambda *a, **k: EchoToShape.apply_model(shim, *a, **k), uc, triples)
    return shim, EchoToShape, ad, O, triples, uc, c, noise1


def case_plms_tiny():
    PLMSSampler = plms_sampler_class()
    out = {}
    for S in (4, 5):
        shim, EchoToShape, ad, O, triples, uc, c, noise1 = _tiny()
        sampler = PLMSSampler(ad)
        states = _record_states(sampler)
        with torch.no_grad():
            z, _ = sampler.sample(S=S, batch_size=O, shape=(3, 16, 16, 16), conditioning=c, x_T=noise1.repeat(O, 1, 1, 1, 1),
                                  verbose=False, eta=0.0)
        assert len(states) == len(sampler.ddim_timesteps) and len(ad.calls) == len(states) + 1
        assert torch.equal(states[-1], z)
        k = 'S%d_' % S
        out[k + 'z_final'] = z
        out[k + 'calls'] = np.array(ad.calls)
        out[k + 'ddim_timesteps'] = np.asarray(sampler.ddim_timesteps)
        out[k + 'states_sub'] = torch.stack([s[:, :, ::4, ::4, ::4] for s in states])
        out[k + 'states_abs'] = np.array([float(s.double().abs().sum()) for s in states])
        print('S=%d calls %s max|z| %.2f' % (S, ad.calls, z.abs().max()))
    save('plms_tiny', uc_s=uc, triples=triples, **out)


def case_plms_keep_tiny():
    PLMSSampler = plms_sampler_class()
    shim, EchoToShape, ad, O, triples, uc, c, noise1 = _tiny()
    x0 = rnd((O, 3, 16, 16, 16), X0_SEED, 0.6)
    table = torch.stack([rnd((O, 3, 16, 16, 16), QNOISE_SEED + k) for k in range(4)])
    mask = torch.zeros(O, 1, 1, 1, 1)
    mask[KEEP] = 1.0
    n = {'i': 0}

    def q(x_start, t, noise=None):
        # q_sample draws with randn_like: hand it the rows of ``table`` instead, in call order
        i = n['i']
        n['i'] += 1
        return EchoToShape.q_sample(shim, x_start, t, noise=table[i].clone())
    ad.q_sample = q
    sampler = PLMSSampler(ad)
    states = _record_states(sampler)
    seen = []
    p_wrapped = sampler.p_sample_plms

    def p(x, *a, **k):
        seen.append(x.clone())
        return p_wrapped(x, *a, **k)
    sampler.p_sample_plms = p
    with torch.no_grad():
        z, _ = sampler.sample(S=4, batch_size=O, shape=(3, 16, 16, 16), conditioning=c, x_T=noise1.repeat(O, 1, 1, 1, 1),
                              verbose=False, eta=0.0, mask=mask, x0=x0)
    assert n['i'] == 4 and len(seen) == 4 and len(ad.calls) == 5
    save('plms_keep_tiny', uc_s=uc, triples=triples, keep=np.array(KEEP), seeds=np.array([X0_SEED, QNOISE_SEED]), z_final=z,
         img_first=seen[0], calls=np.array(ad.calls), states_sub=torch.stack([s[:, :, ::4, ::4, ::4] for s in states]),
         states_abs=np.array([float(s.double().abs().sum()) for s in states]))


def case_scene_plms_tiny():
    import tempfile
    PLMSSampler = plms_sampler_class()
    tmp = tempfile.mkdtemp(prefix='golden_plms_')
    vq = mg._vqvae(32, 64)
    fill(vq, 'e2e.vqvae.')
    vq_path = os.path.join(tmp, 'vq.pth')
    torch.save(vq.state_dict(), vq_path)
    opt = escfg.tiny_diff_opt(device='cpu', logs_dir=tmp, vq_ckpt=vq_path)
    opt.misc.debug = 0
    import model.networks.diffusion_shape.echo2shape as e2s
    e2s.init_mesh_renderer = lambda **k: None
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
    rec = {}

    def rel2shape_plms(data, ddim_eta=0.0):
        """rel2shape (echo2shape.py:484-525) with PLMSSampler in the place of DDIMSampler"""
        S.switch_eval()
        S.set_input(data)
        B = S.rel.shape[0]
        ad = Adapter(S, S.apply_model, S.uc_rel, S.triples)
        samples, _ = PLMSSampler(ad).sample(S=S.ddim_steps, batch_size=B, shape=S.z_shape, conditioning=S.rel,
                                            x_T=noise1.repeat(B, 1, 1, 1, 1), verbose=False, eta=ddim_eta)
        rec['z'], rec['calls'] = samples, list(ad.calls)
        S.gen_df = S.vqvae_module.decode_no_quant(samples)
        return S.gen_df
    S.rel2shape = rel2shape_plms
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
    out = dict(objs=objs, triples=triples, z=rec['z'], calls=np.array(rec['calls']), shapes=d['shapes'][:, :, ::4, ::4, ::4],
               shapes_abs=d['shapes'].double().abs().sum())
    for k in ('sizes', 'translations', 'angles'):
        out[k] = d[k]
    save('scene_plms_tiny', **out)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--only', default=None)
    ap.add_argument('--ref', required=True, help='checkout of the reference (read-only)')
    args = ap.parse_args()
    mg.install_reference(args.ref)
    cases = dict(plms_tiny=case_plms_tiny, plms_keep_tiny=case_plms_keep_tiny, scene_plms_tiny=case_scene_plms_tiny)
    for name, fn in cases.items():
        if args.only in (None, name):
            fn()
