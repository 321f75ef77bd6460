#!/usr/bin/env python
"""ms per DDIM layout iteration against ms per default (ancestral) layout iteration of the same build: the bench's layout denoiser
(model_channels 512), two LayoutDenoisers on ONE set of packed weights, both plans replayed as captured graphs, repetitions
interleaved (DDPM, DDIM, DDPM, ...).  The two plans differ in their last op (es_ddpm_update / es_ddim_rows_update) and in the length
of their per-iteration tables only.  Also prints the device memory with one and with both denoisers resident.
usage: python tools/layout_ddim_step_times.py [--objects 32] [--steps 100] [--reps 7]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from echoscene_amd import synth, config as escfg                       # noqa: E402
from echoscene_amd.model.unet import UNet1DModel                       # noqa: E402
from echoscene_amd.samplers import LayoutDenoiser                      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--objects', type=int, default=32)
ap.add_argument('--steps', type=int, default=100)
ap.add_argument('--reps', type=int, default=7)
a = ap.parse_args()
dev = torch.device('cuda')
net = UNet1DModel(**escfg.layout_denoiser_kwargs(512))
synth.seeded_fill_(net, prefix='bench.layout.')
dk = escfg.layout_diffusion_kwargs(1000)
gb = lambda: torch.cuda.memory_allocated() / 2 ** 30
dens = {'ddpm': LayoutDenoiser(net, dk, dev)}
m1 = gb()
dens['ddim'] = LayoutDenoiser(net, dk, dev, sampler='ddim', steps=a.steps, weights=dens['ddpm'].w)
m2 = gb()
O = a.objects
objs, triples = synth.synthetic_graph(O, seed=5)
oe = torch.randn(O, 640, generator=torch.Generator().manual_seed(6))
states = {}
for name, den in dens.items():
    den.sample(oe, triples, n_steps=3)                                 # builds the plan, captures its graph
    states[name] = den._last
torch.cuda.synchronize()
print('device memory: %.3f GB with the default denoiser, %.3f GB with the DDIM denoiser as well (+%.1f MB), %.3f GB with both plans'
      % (m1, m2, (m2 - m1) * 1024, gb()))
ms = {name: [] for name in dens}
for _ in range(a.reps):
    for name, st in states.items():
        st['x'].copy_(st['noise'][0])
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        st['plan'].sample(st['step'], 0, a.steps, use_graph=True)
        e1.record()
        torch.cuda.synchronize()
        ms[name].append(e0.elapsed_time(e1) / a.steps)
for name in ms:
    xs = sorted(ms[name])
    print('%s: ms per iteration median %.4f min %.4f max %.4f (%d reps x %d iterations, O = %d, %d launches per iteration)'
          % (name, xs[len(xs) // 2], xs[0], xs[-1], a.reps, a.steps, O, states[name]['plan'].n_launches))
d, p = sorted(ms['ddim'])[a.reps // 2], sorted(ms['ddpm'])[a.reps // 2]
print('ddim / ddpm = %.4f' % (d / p))
