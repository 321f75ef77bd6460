#!/usr/bin/env python
"""Golden vectors of strided DDIM sampling of the LAYOUT loop, from the REFERENCE ITSELF (read-only): its model-agnostic
``DDIMSampler`` (model/networks/diffusion_shape/samplers/ddim.py) driven on the layout denoiser ``DiffusionPoint._denoise``.

    python tests/golden/make_golden_layout_ddim.py --ref <checkout of the reference> [--only NAME]

Loads make_golden.py for its helpers (reference import with stand-ins, seeded fill, save) and stores numbers only.  The reference has
no strided layout sampler of its own; two things make its DDIMSampler run on the layout model, none of which touches its arithmetic:
  * ``DDIMSampler.register_buffer`` moves every table to 'cuda': replaced by a plain setattr, as make_golden.py does;
  * an adapter in front of ``DiffusionPoint`` exposes what the sampler touches of its model -- ``num_timesteps``, ``alphas_cumprod``,
    ``alphas_cumprod_prev``, ``betas``, ``device`` (the tables of the layout ``GaussianDiffusion``), ``apply_model(x, uc, triplet, t, c)``
    forwarded to ``_denoise(x.reshape(O, 8), uc, triplet, t, c).reshape(O, 8, 1, 1)`` and ``q_sample(x0, t)`` forwarded to
    ``GaussianDiffusion.q_sample`` with injected draws.
The sampler is called as ``sample(S, batch_size=O, shape=(8, 1, 1), x_T=..., unconditional_guidance_scale=3.,
unconditional_conditioning=obj_embed, triplet=triples, eta=...)``: the ``elif True`` branch of p_sample_ddim, one evaluation, no
guidance.  The eta draws are injected through ``noise_like``.

  layout_ddim_tiny: the model and graph of layout_loop_tiny (O = 8, width 128) with T = 1000 trained timesteps.  S = 4 and S = 5 at
      eta 0, S = 4 at eta 0.7, S = 100 at eta 0: final x, the state after every iteration (S <= 5), the timesteps the denoiser was
      called at, and the schedule tables (ddim_alphas, ddim_alphas_prev, ddim_sqrt_one_minus_alphas, ddim_sigmas) for S = 4, 5, 100
      at eta 0 and 0.7.  ``noise`` [6, O, 8]: row 0 = x_T of every run, rows 1 + i the injected eta draws of iteration i.
  layout_ddim_full: width 512, the loop inputs of unet1d_full (O = 8), S = 10, eta 0: final x and the state after iteration 0.
  layout_ddim_keep_tiny: O = 4, nodes [1, 3] kept, S = 4, ``mask`` / ``x0`` and injected q_sample draws: the blended state in front of
      iteration 0 and the final x.
  scene_layout_ddim_tiny: the scene call of scene_e2e_tiny with the reference's layout loop replaced by the adapter run (S = 4), for
      'echolayout' and for 'echoscene' with gen_shape=False.
"""
import argparse
import importlib.util
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location('make_golden', os.path.join(HERE, 'make_golden.py'))
mg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mg)
synth, escfg, fill, rnd, save = mg.synth, mg.escfg, mg.fill, mg.rnd, mg.save

KEEP = [1, 3]                 # kept nodes of layout_ddim_keep_tiny (O = 4)
X0_SEED, QNOISE_SEED = 81, 2950


def ddim_sampler_class():
    from model.networks.diffusion_shape.samplers.ddim import DDIMSampler
    DDIMSampler.register_buffer = lambda self, name, attr: setattr(self, name, attr)
    return DDIMSampler


class Adapter:
    """what DDIMSampler touches of its model, on a layout DiffusionPoint"""

    def __init__(self, df, q_table=None):
        gd = df.diffusion
        self._df, self._gd = df, gd
        self.num_timesteps = gd.num_timesteps
        self.alphas_cumprod, self.alphas_cumprod_prev, self.betas = gd.alphas_cumprod, gd.alphas_cumprod_prev, gd.betas
        self.device = torch.device('cpu')
        self.calls = []
        self._q_table, self._q_n = q_table, 0

    def apply_model(self, x, uc, triplet, t, c):
        O = x.shape[0]
        self.calls.append(int(t[0]))
        assert bool((t == t[0]).all()) and tuple(x.shape) == (O, 8, 1, 1)
        return self._df._denoise(x.reshape(O, 8), uc, triplet, t, c).reshape(O, 8, 1, 1)

    def q_sample(self, x0, t):
        # q_sample draws with torch.randn: hand it the rows of the table instead, in call order
        i = self._q_n
        self._q_n += 1
        return self._gd.q_sample(x0, t, noise=self._q_table[i].clone())


def run(df, S, x_T, oe, triples, eta=0.0, draws=None, mask=None, x0=None, q_table=None):
    """DDIMSampler.sample through the adapter; returns (x [O, 8], states after every iteration, states in front of every iteration,
    the timesteps the denoiser was called at, the sampler)"""
    from model.networks.diffusion_shape.samplers import ddim as ddim_mod
    O = x_T.shape[0]
    ad = Adapter(df, q_table)
    sampler = ddim_sampler_class()(ad)
    after, before = [], []
    p_orig = sampler.p_sample_ddim

    def p(x, *a, **k):
        before.append(x.reshape(O, 8).clone())
        outs = p_orig(x, *a, **k)
        after.append(outs[0].reshape(O, 8).clone())
        return outs
    sampler.p_sample_ddim = p
    n = {'i': 0}
    _orig = ddim_mod.noise_like

    def nl(shape, device, repeat=False):
        k = n['i']
        n['i'] += 1
        assert tuple(shape) == (O, 8, 1, 1) and not repeat
        # (eta = 0: sigma_t = 0 multiplies whatever is returned; zeros keep the run free of the global generator)
        return draws[k].reshape(O, 8, 1, 1).clone() if draws is not None else torch.zeros(shape)
    ddim_mod.noise_like = nl
    try:
        with torch.no_grad():
            x, _ = sampler.sample(S, batch_size=O, shape=(8, 1, 1), x_T=x_T.reshape(O, 8, 1, 1).clone(), verbose=False,
                                  unconditional_guidance_scale=3., unconditional_conditioning=oe, triplet=triples, eta=eta,
                                  mask=None if mask is None else mask.reshape(O, 1, 1, 1),
                                  x0=None if x0 is None else x0.reshape(O, 8, 1, 1))
    finally:
        ddim_mod.noise_like = _orig
    assert len(after) == len(sampler.ddim_timesteps) == len(ad.calls) and n['i'] == len(after)
    assert torch.equal(after[-1], x.reshape(O, 8))
    return x.reshape(O, 8), after, before, ad.calls, sampler


def _tables(df, S, eta):
    s = ddim_sampler_class()(Adapter(df))
    s.make_schedule(ddim_num_steps=S, ddim_eta=eta, verbose=False)
    t = lambda v: torch.as_tensor(np.asarray(v))
    return dict(ddim_timesteps=np.asarray(s.ddim_timesteps), ddim_alphas=t(s.ddim_alphas), ddim_alphas_prev=t(s.ddim_alphas_prev),
                ddim_sqrt_one_minus_alphas=t(s.ddim_sqrt_one_minus_alphas), ddim_sigmas=t(s.ddim_sigmas))


def _layout_model(mc, ctx, prefix, time_num=1000):
    from model.networks.diffusion_layout.diffusion_ddpm import DiffusionPoint
    net, kw = mg._unet1d(mc, ctx)
    fill(net, prefix)
    return DiffusionPoint(denoise_net=net, config=escfg.AttrDict(angle_dim=2), **dict(escfg.layout_diffusion_kwargs(time_num)))


def case_layout_ddim_tiny():
    df = _layout_model(128, 128, 'unet1d_tiny.')
    O = 8
    objs, triples = synth.synthetic_graph(O, seed=3)
    oe = rnd((O, 640), 100 + 3)
    plain = np.load(os.path.join(HERE, 'layout_loop_tiny.npz'))
    assert np.array_equal(plain['obj_embed'], oe.numpy()) and np.array_equal(plain['triples'], triples.numpy())
    noise = synth.layout_noise(O, 8, 5, seed=7)                  # row 0 = x_T, rows 1 + i = the eta draws of iteration i
    out = dict(obj_embed=oe, triples=triples, noise=noise)
    for S, eta, tag in ((4, 0.0, 'S4'), (5, 0.0, 'S5'), (4, 0.7, 'S4_eta07'), (100, 0.0, 'S100')):
        x, after, _, calls, _ = run(df, S, noise[0], oe, triples, eta=eta, draws=noise[1:] if eta else None)
        out[tag + '_x_final'] = x
        out[tag + '_calls'] = np.array(calls)
        if S <= 5:
            out[tag + '_states'] = torch.stack(after)
        print('%s: calls %s max|x| %.3f' % (tag, calls if S <= 5 else '%d..%d' % (calls[0], calls[-1]), x.abs().max()))
    for S in (4, 5, 100):
        for eta, et in ((0.0, 'eta0'), (0.7, 'eta07')):
            for k, v in _tables(df, S, eta).items():
                out['tab_S%d_%s_%s' % (S, et, k)] = v
    gd = df.diffusion
    out.update(sac1000=gd.sqrt_alphas_cumprod, s1mac1000=gd.sqrt_one_minus_alphas_cumprod)
    save('layout_ddim_tiny', **out)


def case_layout_ddim_full():
    df = _layout_model(512, 1280, 'unet1d_full.')
    O = 8
    objs, triples = synth.synthetic_graph(O, seed=4)
    oe = rnd((O, 640), 100 + 4)
    full = np.load(os.path.join(HERE, 'unet1d_full.npz'))
    assert np.array_equal(full['loop_obj_embed'], oe.numpy()) and np.array_equal(full['loop_triples'], triples.numpy())
    x_T = synth.layout_noise(O, 8, 1000, seed=7)[0]
    x, after, _, calls, _ = run(df, 10, x_T, oe, triples)
    save('layout_ddim_full', x_T=x_T, x_final=x, x_iter0=after[0], calls=np.array(calls))


def case_layout_ddim_keep_tiny():
    df = _layout_model(128, 128, 'unet1d_tiny.')
    O, S = 4, 4
    objs, triples = synth.synthetic_graph(O, seed=6)
    oe = rnd((O, 640), 100 + 6)
    x_T = synth.layout_noise(O, 8, S, seed=7)[0]
    x0 = torch.zeros(O, 8)
    x0[KEEP] = rnd((len(KEEP), 8), X0_SEED, 0.5)
    table = torch.stack([rnd((O, 8), QNOISE_SEED + k) for k in range(S)])
    mask = torch.zeros(O)
    mask[KEEP] = 1.0
    x, after, before, calls, _ = run(df, S, x_T, oe, triples, mask=mask, x0=x0, q_table=table.reshape(S, O, 8, 1, 1))
    plain, _, _, _, _ = run(df, S, x_T, oe, triples)
    gen = [i for i in range(O) if i not in KEEP]
    d = (x[gen] - plain[gen]).abs().amax(dim=1)
    print('layout_ddim_keep_tiny: per generated row, max |masked - unmasked| =', ['%.3e' % v for v in d.tolist()])
    assert float(d.min()) > 1e-3, 'the kept nodes do not act as context: choose other nodes / x0'
    save('layout_ddim_keep_tiny', obj_embed=oe, triples=triples, keep=np.array(KEEP), seeds=np.array([X0_SEED, QNOISE_SEED]), x_T=x_T,
         x0=x0, keep_noise=table, img_first=before[0], x_final=x, x_final_unmasked=plain, calls=np.array(calls))


def case_scene_layout_ddim_tiny():
    import model.networks.diffusion_layout.diffusion_ddpm as dd
    out = {}
    S = 4
    _orig_gen = dd.DiffusionPoint.gen_samples_sg
    rec = {}

    def gen(self_, shape, device, obj_embed, triples=None, condition=None, noise_fn=None, clip_denoised=True, keep_running=False, **kw):
        """gen_samples_sg with DDIMSampler through the adapter in the place of p_sample_loop_sg"""
        assert not clip_denoised
        x, _, _, calls, _ = run(self_, S, rec['x_T'], obj_embed, triples)
        rec['calls'] = calls
        return x
    dd.DiffusionPoint.gen_samples_sg = gen
    try:
        for typ, tag in (('echolayout', 'lay_'), ('echoscene', 'sc_')):
            h = mg._SGDiffHarness(typ, False)
            rec['x_T'] = h.noise[0]
            with torch.no_grad():
                d = h.m.sample_box_and_shape(h.objs, h.triples, h.tf, h.rf, gen_shape=False)
            for k in ('sizes', 'translations', 'angles'):
                out[tag + k] = d[k]
            out[tag + 'calls'] = np.array(rec['calls'])
            out.update(objs=h.objs, triples=h.triples)
    finally:
        dd.DiffusionPoint.gen_samples_sg = _orig_gen
    save('scene_layout_ddim_tiny', **out)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--only', default=None)
    ap.add_argument('--ref', required=True, help='checkout of the reference (read-only)')
    args = ap.parse_args()
    mg.install_reference(args.ref)
    cases = dict(layout_ddim_tiny=case_layout_ddim_tiny, layout_ddim_full=case_layout_ddim_full,
                 layout_ddim_keep_tiny=case_layout_ddim_keep_tiny, scene_layout_ddim_tiny=case_scene_layout_ddim_tiny)
    for name, fn in cases.items():
        if args.only in (None, name):
            fn()
