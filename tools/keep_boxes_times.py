"""Timing of box-preserving sampling, one configuration per process (HIP events, median of 7 runs after a discarded warm-up run):

    python tools/keep_boxes_times.py layout [O]           one layout step, unmasked: bench width (model_channels 512), T = 1000, one
                                                          captured graph per step, a run = the whole 1000-step loop
    python tools/keep_boxes_times.py layout-masked [O]    the same with every second node kept (the keep plan)
    python tools/keep_boxes_times.py scene [O]            sample_box_and_shape(gen_shape=True) at full width, without box keeping
    python tools/keep_boxes_times.py scene-masked [O]     ... with every second node's box kept

``layout`` needs nothing of this feature, so the same file times the tree of the commit before it (the figure the others are read
against).  Run each line in a process of its own and the whole sequence twice: the spread of the parent's repeated runs is the margin."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.getcwd())            # the tree the process was started in (this one, or a checkout of the parent commit)
import bench  # noqa: E402
from echoscene_amd import synth, config as escfg  # noqa: E402

mode = sys.argv[1] if len(sys.argv) > 1 else 'layout'
O = int(sys.argv[2]) if len(sys.argv) > 2 else 32
RUNS = 7
dev = torch.device('cuda')


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def report(name, ts, per):
    ts = sorted(t / per for t in ts)
    print('%s: median %.4f ms (min %.4f - max %.4f) over %d runs' % (name, float(np.median(ts)), ts[0], ts[-1], len(ts)), flush=True)


if mode in ('layout', 'layout-masked'):
    net, den, obj_embed, triples = bench.build_layout(dev, O, seed=100)
    T = den.T
    kw = {}
    if mode == 'layout-masked':
        mask = torch.zeros(O)
        mask[::2] = 1.0
        kw = dict(x0=torch.from_numpy(np.random.RandomState(1).uniform(-1, 1, (O, 8)).astype(np.float32)), mask=mask)
    den.sample(obj_embed, triples, noise=None, n_steps=5, **kw)          # plan build + graph capture
    st = den._last
    plan = st['plan']
    loop = lambda: plan.sample(st['step'], 0, T)
    timed(loop)                                                           # the discarded warm-up run
    ts = [timed(loop) for _ in range(RUNS)]
    report('%s O=%d T=%d, %d ops, %d launches per step; per step' % (mode, O, T, plan.n_ops, plan.n_launches), ts, T)
else:
    from model.SGDiff import SGDiff
    opt = escfg.default_diff_opt('cuda', concat=False)
    m = SGDiff('echoscene', opt, synth.VOCAB, replace_latent=False, with_changes=True, residual=True, gconv_pooling='avg',
               with_angles=True, clip=True, separated=False)
    synth.seeded_fill_(torch.nn.Module.state_dict(m.diff), prefix='lat.diff.')
    synth.seeded_fill_(m.diff.ShapeDiff.df, prefix='lat.df.')
    synth.seeded_fill_(m.diff.ShapeDiff.vqvae, prefix='lat.vq.')
    m.diff.optimizer_ini()
    m.cuda()
    m.eval()
    objs, triples = synth.synthetic_graph(O, seed=20)
    tf, rf = synth.synthetic_features(O, triples.shape[0], seed=20)
    a = (objs.cuda(), triples.cuda(), tf.cuda(), rf.cuda())
    kw = {}
    if mode == 'scene-masked':
        nodes = list(range(0, O, 2))
        kw = dict(keep_box_nodes=nodes,
                  keep_boxes=torch.from_numpy(np.random.RandomState(1).uniform(-1, 1, (len(nodes), 8)).astype(np.float32)))
    call = lambda: m.sample_box_and_shape(*a, gen_shape=True, **kw)
    call()
    timed(call)
    ts = [timed(call) for _ in range(3)]
    report('%s O=%d, whole call' % (mode, O), ts, 1)
