"""Loop owners on the host side: thin objects that own packed weights + per-graph plans and call
the native sampling loop.  They mirror ``EchoToLayout`` / ``EchoToShape`` of the reference
(model/networks/diffusion_layout/echo2layout.py, diffusion_shape/echo2shape.py)."""
import math
import os

import torch

from . import hip
from .plan import (Builder, GraphIndex, View, GCNWeights, UNet1DWeights, emit_gcn, emit_unet1d_step, time_tables, sub_plan)
from .plan_vol import UNet3DWeights, emit_unet3d_step, VQWeights, emit_vq_decode, VQEncWeights, emit_vq_encode
from .schedules import LayoutSchedule, LayoutDdimSchedule, ShapeSchedule, timestep_embedding_table, SHAPE_SAMPLERS, LAYOUT_SAMPLERS


def _cap(n_triples):
    """triple-row capacity class of a plan (GraphIndex): the count rounded up to a multiple of 32"""
    return max(32, (int(n_triples) + 31) // 32 * 32)


def state_dict_for(module, device=None):
    """The module's state dict as the weight planners read it.  Entries that already live on ``device`` (a GPU) stay there: the
    fp64 folds and the weight re-layouts then run on the GPU from the parameters in place -- a model moved with ``.cuda()`` used to be
    downloaded tensor by tensor (1867 copies), folded on the host and uploaded again (1300 copies), 1.5 s of a process's first scene
    call.  Everything else comes to the host.  The planners never keep an entry itself (plan.own)."""
    dev = None if device is None else torch.device(device)
    on_dev = lambda v: dev is not None and dev.type == 'cuda' and v.is_cuda and (dev.index is None or v.device.index == dev.index)
    return {k: (v.detach() if on_dev(v) else v.detach().cpu()) for k, v in module.state_dict().items()}


def _cpu_sd(module):
    return state_dict_for(module, None)


def gcn_forward(sd, prefix, obj, pred, triples, device=None, weights=None, pooling='avg'):
    """GraphTripleConvNet.forward on the HIP path (setup GCNs and unit tests).
    obj f32[O,Dobj], pred f32[T,Dp] (any device), triples int64[T,3] -> (obj_out, pred_out) on device."""
    device = device or torch.device('cuda')
    gw = weights or GCNWeights(sd, prefix, device, pooling)
    g = GraphIndex(triples, obj.shape[0], device)
    b = Builder(device)
    o = b.dev(obj)
    p = b.dev(pred)
    oo, po = emit_gcn(b, gw, g, View(o), obj.shape[1], View(p), pred.shape[1], want_pred=True)
    plan = b.finish()
    plan.run()
    torch.cuda.synchronize()
    out_p = po.t if po.col == 0 and po.ld == po.t.shape[1] else po.t[:, po.col:po.col + po.width].contiguous()
    return oo.t, out_p


# emit / compose / stage: EMIT a loop step's ops on any Builder (no denoiser, no device: the CPU tests plan with the same
# functions), COMPOSE the op list into a state's named plans, STAGE a call's inputs into the state in a fixed order of the device draws
SUB_PLANS = ('plan', 'eps_plan', 'stem_plan', 'main_plan', 'first_plan', 'main_a_plan', 'stem2_plan', 'main_b_plan')
STATE_KEYS = SUB_PLANS + ('x', 'eps', 'step', 'noise', 'snoise', 'x0', 'mask', 'knoise', 'objbuf', 'lo', 'hi', 'O', 'g', 'pred', 'sig',
                          'sampler', 'codes_local', 'codes_all', 'code_cols', 'xc', 'cdev', 'oe_w', 'ucw')


def new_state(**kw):
    """a plan state with EVERY key present (None where a plan has no such buffer or sub-plan) and ``empty`` False"""
    st = dict.fromkeys(STATE_KEYS)
    st['empty'] = False
    st.update(kw)
    return st


def emit_layout_step(b, w, g, obj_embed, temb, tables, T, coef=None, keep_tab=None, clip=False, keep=False, eps_out=None,
                     sampler='ddpm', step_noise=True):
    """The layout loop step on ``b``: one UNet1D evaluation on x [O, 8] at the iteration ``step`` counts, then -- with the schedule's
    ``coef`` table -- the ancestral update (``keep``: es_ddpm_update_keep, which also carries the kept rows; it reads ``keep_tab``).
    ``T``: the iterations of the loop (rows of the noise and keep tables).  ``clip``: clip_denoised of the update.  ``coef=None``: the
    denoiser alone; ``eps_out``: a plain eps tensor instead of the output conv's K slices.
    ``sampler='ddim'``: the same ops with the LAST one replaced by the strided DDIM update (es_ddim_rows_update, masked or not; ``coef``
    = LayoutDdimSchedule.coef); it reads the per-iteration draws only with ``step_noise`` (eta != 0).
    Buffers are allocated in a fixed order; returns them by name (``n_eps_ops``: the ops in front of the update)."""
    if sampler not in LAYOUT_SAMPLERS:
        raise ValueError('sampler must be one of %s, got %r' % (LAYOUT_SAMPLERS, sampler))
    if sampler == 'ddim' and clip:
        raise ValueError('layout DDIM: clip_denoised=True has no reference arithmetic under DDIM (p_sample_ddim never clips)')
    O, D = g.O, w.in_ch
    x = b.buf(O, D)
    step = b.buf(1, dtype=torch.int32, zero=True)
    noise = b.buf(T + 1, O, D)
    oe = b.dev(obj_embed)
    objbuf, pred = emit_unet1d_step(b, w, g, x, oe, temb, step, eps_out, tables=tables)
    eps = b.tags['eps']                                  # View: the output conv's K slices (the update sums the slabs)
    out = dict(x=x, step=step, noise=noise, objbuf=objbuf, oe_w=oe.shape[1], eps=eps, n_eps_ops=len(b.ops), pred=pred)
    if coef is None:
        return out
    draws = View(noise[1:].reshape(T, O * D), ld=O * D)
    if keep:
        out.update(x0=b.buf(O, D, zero=True), mask=b.buf(O, zero=True), knoise=b.buf(T, O * D, zero=True))
    if sampler == 'ddim':
        kw = dict(x0=out['x0'], mask=out['mask'], keep_noise=out['knoise'], tab=keep_tab) if keep else {}
        b.ddim_rows(x, eps, coef, step, noise=draws if step_noise else None, noise_stride=O * D if step_noise else 0, inc_step=True, **kw)
    elif keep:
        b.update_keep(x, eps, coef, step, draws, O * D, out['x0'], out['mask'], out['knoise'], keep_tab, inc_step=True, clip_x0=clip)
    else:
        b.update(hip.OP_DDPM, x, eps, coef, step, noise=draws, noise_stride=O * D, inc_step=True, clip_x0=clip)
    return out


def emit_shape_step(b, w, g, uc, temb, tables, coef, keep_tab, S, z_shape, lo, hi, c_local=None, gather_rows=None, keep=False,
                    plms=False, step_noise=False, keep_vox=False):
    """The shape loop step on ``b`` for the objects lo:hi of the graph: the blend of the masked loop (``keep``; the reference blends
    before p_sample_ddim, samplers/ddim.py:160-163: the denoiser -- conv-pool stem and shape GCN included -- reads the kept objects'
    forward-noised latents), one UNet3D evaluation, then the sampler's tail: es_ddim_update, the same with the per-step draws
    (``step_noise``: eta != 0), or es_plms_update (``plms``; its two first-iteration ops are returned as ``first_ops``, not appended).
    ``keep_vox``: the voxel form of the masked loop (shape completion) -- ``mask`` is [Ol, V], one value per latent voxel, and the one
    op in front of the denoiser is es_ddim_blend_vox instead of es_ddim_blend; everything else is the ``keep`` step.
    The sharding hints (shard_block, force_exchange, o_hint) and the precision are those ``b`` was made with.  ``temb`` is not read
    (the time tables hold what it fed); it keeps its place for the callers."""
    keep = bool(keep or keep_vox)
    x = b.buf(hi - lo, *z_shape)
    eps = b.buf(hi - lo, *z_shape)
    step = b.buf(1, dtype=torch.int32, zero=True)
    out = dict(x=x, eps=eps, step=step, n_blend=1 if keep else 0, first_ops=(None, None))
    if keep:
        mshape = (hi - lo, math.prod(int(d) for d in z_shape[1:])) if keep_vox else (hi - lo,)
        out.update(x0=b.buf(hi - lo, *z_shape, zero=True), mask=b.buf(*mshape, zero=True), knoise=b.buf(S, x.numel(), zero=True))
        (b.blend_vox if keep_vox else b.blend)(x, out['x0'], out['mask'], out['knoise'], keep_tab, step)
    ucd = b.dev(uc)
    r = emit_unet3d_step(b, w, g, x, ucd, step, eps, tables, dims=z_shape[1:], lo=lo, hi=hi, c_dev=c_local, gather_rows=gather_rows)
    out.update(objbuf=r.objbuf, ucw=ucd.shape[1], n_eps_ops=len(b.ops), split=r.split, codes_local=r.codes_local,
               codes_all=r.codes_all, code_cols=r.code_cols, xc=r.xc, cdev=r.cdev, pred=r.pred_rows)
    if plms:
        # the sampler's state: the last three eps, iteration i in slot i % 3, and x at the start of iteration 0
        ring, xsave = b.buf(3, x.numel(), zero=True), b.buf(x.numel(), zero=True)
        out['first_ops'] = (b.plms(hip.OP_PLMS_FIRST_A, x, eps, coef, step, ring, xsave, push=False),
                            b.plms(hip.OP_PLMS_FIRST_B, x, eps, coef, step, ring, xsave, push=False))
        b.plms(hip.OP_PLMS, x, eps, coef, step, ring, xsave, inc_step=True)
    elif step_noise:
        nz = x.numel()
        out['snoise'] = b.buf(S, nz)
        b.update(hip.OP_DDIM, x, eps, coef, step, noise=View(out['snoise'], ld=nz), noise_stride=nz, inc_step=True)
    else:
        b.update(hip.OP_DDIM, x, eps, coef, step, inc_step=True)
    return out


def compose_step_plans(ops, n_blend, split, n_eps_ops, first_a, first_b, plms=False, sharded=False):
    """The op lists of a shape plan state's sub-plans, by name (SUB_PLANS; None: this state has no such plan).  ``ops``: the steady
    step = ``n_blend`` blend ops, the denoiser (the echo exchange sits in front of op ``split``), one sampler op behind ``n_eps_ops``.
    ``sharded``: 'stem_plan' + 'main_plan' = the step cut at the exchange.  ``plms``: 'first_plan' is iteration 0 -- the step with
    ``first_a`` for the sampler op, then the denoiser once more (no blend: the reference blends once per iteration) with ``first_b``;
    sharded, its two passes are stem -> 'main_a_plan' and 'stem2_plan' (the stem without the blend) -> 'main_b_plan'."""
    out = dict.fromkeys(SUB_PLANS)
    out['plan'], out['eps_plan'] = ops, ops[:n_eps_ops]
    if sharded:
        out['stem_plan'], out['main_plan'] = ops[:split], ops[split:]
    if plms:
        out['first_plan'] = ops[:n_eps_ops] + [first_a] + ops[n_blend:n_eps_ops] + [first_b]
        if sharded:
            out['main_a_plan'] = ops[split:n_eps_ops] + [first_a]
            out['stem2_plan'] = ops[n_blend:split] if n_blend else out['stem_plan']
            out['main_b_plan'] = ops[split:n_eps_ops] + [first_b]
    return out


def _check_keep_pair(x0, mask, keep_noise, loop, arg=''):
    """x0 and mask go together, and keep_noise needs them (``arg``: the prefix the caller's keywords carry)"""
    if (mask is None) != (x0 is None):
        raise ValueError('%s needs both %sx0 and %smask' % (loop, arg, arg))
    if mask is None and keep_noise is not None:
        raise ValueError('%skeep_noise without a %smask' % (arg, arg))


def _check_mask(x0, mask, shape, loop, form, unit, per=1):
    """mask [O] of zeros and ones and x0 of ``shape`` = [O, ...] for the masked loop ``loop``; returns (x0, mask f32 [O]).
    ``per`` > 1: a mask of ``per`` values for each object, returned as it is, [O, per]"""
    mask = torch.as_tensor(mask, dtype=torch.float32)
    mask = mask.reshape(-1) if per == 1 else mask
    x0 = torch.as_tensor(x0)
    if mask.numel() != shape[0] * per or tuple(x0.shape) != tuple(shape):
        raise ValueError('%s: x0 must be %s = %s and mask [O]; got %s and %d entries' % (loop, form, tuple(shape), tuple(x0.shape), mask.numel()))
    if not bool(((mask == 0) | (mask == 1)).all()):
        raise ValueError('%s: the mask is per %s, 0 (generate) or 1 (keep)' % (loop, unit))
    return x0, mask


def _check_shape_mask(x0, mask, O, z_shape):
    """mask and x0 of the masked shape loop -> (x0, mask f32, vox).  The mask is per object -- [O] -> f32 [O], vox False -- or per latent
    voxel, shared by the channels -- [O, 1, D, H, W] or [O, D, H, W] -> f32 [O, D * H * W], vox True.  Anything else (a per-channel
    mask [O, C, D, H, W] too) is refused."""
    z_shape = tuple(int(d) for d in z_shape)
    zd = z_shape[1:]
    m = torch.as_tensor(mask, dtype=torch.float32)
    if tuple(m.shape) in ((O, 1) + zd, (O,) + zd, (O, math.prod(zd))):          # (the last: the flattened form the plan's buffer has)
        return _check_mask(x0, m.reshape(O, -1), (O,) + z_shape, 'masked DDIM', '[O, C, D, H, W]', 'voxel', per=math.prod(zd)) + (True,)
    if m.numel() != O:
        raise ValueError('masked DDIM: the mask is per object, [O] = [%d], or per latent voxel, [O, 1, D, H, W] / [O, D, H, W] with '
                         '(D, H, W) = %s -- one value for all channels; got %s (a mask per channel is not supported)'
                         % (O, zd, tuple(m.shape)))
    return _check_mask(x0, m, (O,) + z_shape, 'masked DDIM', '[O, C, D, H, W]', 'object') + (False,)


class LayoutDenoiser:
    """UNet1DModel + GaussianDiffusion sampling on the HIP path (loop A of SURVEY.md section 3.1)."""

    def __init__(self, net, diffusion_kwargs, device=None, sampler='ddpm', steps=None, eta=0.0, weights=None):
        """``sampler``: 'ddpm' (the shipped ancestral loop over all T trained timesteps) or 'ddim' -- the reference's model-agnostic
        DDIMSampler (samplers/ddim.py) on a strided schedule of ``steps`` of them (schedules.LayoutDdimSchedule), ``eta`` scaling its
        per-step noise (0: deterministic).  A DDIM denoiser has its own, S-row, time-embedding table and ``time_tables``.
        ``weights``: the packed UNet1DWeights of another LayoutDenoiser of the same network and device (another sampler or step count
        does not need a second copy of them)."""
        if sampler not in LAYOUT_SAMPLERS:
            raise ValueError('layout_sampler must be one of %s, got %r' % (LAYOUT_SAMPLERS, sampler))
        if sampler == 'ddpm' and (steps is not None or float(eta or 0.0) != 0.0):
            raise ValueError("layout_steps / layout_eta need layout_sampler='ddim' (the ancestral loop runs every trained timestep)")
        if sampler == 'ddim' and steps is None:
            raise ValueError("layout_sampler='ddim' needs layout_steps")
        self.sampler, self.eta = sampler, float(eta or 0.0)
        self.device = device or torch.device('cuda')
        self.net = net
        dk = dict(diffusion_kwargs)
        if sampler == 'ddim' and dk.get('model_mean_type', 'eps') != 'eps':
            raise ValueError("layout DDIM: model_mean_type=%r has no reference arithmetic under DDIM" % (dk.get('model_mean_type'),))
        self.w = weights if weights is not None else UNet1DWeights(state_dict_for(net, self.device), net, self.device)
        # every parameterisation GaussianDiffusion can sample with is a coefficient table of the same update op (schedules.py)
        self.sched = LayoutSchedule(dk.get('time_num', 1000), dk.get('beta_start', 1e-4), dk.get('beta_end', 0.02),
                                    dk.get('schedule_type', 'linear'), dk.get('model_mean_type', 'eps'),
                                    dk.get('model_var_type', 'fixedsmall'))
        self.T = self.sched.time_num                                # the model's trained timestep count
        if sampler == 'ddim':
            self.sched = LayoutDdimSchedule(self.sched, steps, self.eta)
        self.n_iter = len(self.sched.timesteps)                     # iterations of the loop (T for the ancestral loop)
        self.temb = timestep_embedding_table(self.sched.timesteps, net.model_channels).to(self.device)
        self.coef = self.sched.coef.to(self.device)
        self.keep_tab = self.sched.keep_tab.to(self.device)      # masked loop: q_sample's factors per iteration (es_ddpm_update_keep)
        # time MLP / emb projections / box_time_emb for every step of the schedule (node-independent)
        self.tables = time_tables(self.w, self.temb, self.w.box_t, self.device)
        self._plans, self._last, self.max_plans = {}, None, 4

    def _plan_for(self, obj_embed, triples, clip=False, keep=False):
        """``clip``: clip_denoised=True of p_sample_loop_sg (the predicted x0 clamped to [-1, 1], diffusion_ddpm.py:243-244) -- a
        property of the plan's update op, so it is part of the cache key.
        ``keep``: the plan of the MASKED loop (keep given boxes) -- the same ops with the LAST one, the update, replaced by the update
        that also carries the kept rows (es_ddpm_update_keep), and its inputs ``x0`` [O, 8], ``mask`` [O], ``knoise`` [T, O * 8].  A
        cache entry of its own, as 'clip' is (the two combine): without a mask the plan is, op for op, what it has always been.
        Plans are cached by (node count, triple-row capacity): a NEW scene graph of the same size class only rewrites the
        index arrays and the predicate-embedding rows in place (GraphIndex.update) -- no plan rebuild, no graph re-capture
        (0.3 s per scene in round 1).  Capacity = triple count rounded up to a multiple of 32."""
        O = obj_embed.shape[0]
        cap = _cap(triples.shape[0])
        key = (O, cap) + (('clip',) if clip else ()) + (('keep',) if keep else ())
        sig = hash(triples.detach().cpu().numpy().tobytes())
        st = self._plans.get(key)
        if st is None:
            g = GraphIndex(triples, O, self.device, capacity=cap)
            b = Builder(self.device)
            bufs = emit_layout_step(b, self.w, g, obj_embed, self.temb, self.tables, self.n_iter, self.coef, self.keep_tab, clip, keep,
                                    sampler=self.sampler, step_noise=self.sampler == 'ddpm' or self.eta != 0.0)
            n_eps_ops = bufs.pop('n_eps_ops')
            # 'eps_plan': the same ops minus the update, for step-level parity tests
            st = new_state(plan=b.finish(), eps_plan=sub_plan(b, b.ops[:n_eps_ops]), g=g, sig=sig, **bufs)
            if len(self._plans) >= self.max_plans:               # a few size classes stay resident
                self._plans.pop(next(iter(self._plans)))
            self._plans[key] = st
        elif st['sig'] != sig:
            st['g'].update(triples)
            st['pred'].copy_(self.w.pred_table[torch.from_numpy(st['g'].p_host)])
            st['sig'] = sig
        st['objbuf'][:, :st['oe_w']].copy_(obj_embed.to(self.device))
        self._last = st
        return st

    @property
    def weight_bytes_per_step(self):
        return self._last['plan'].weight_bytes

    def save_model(self, path, obj_embed, triples, keep=False):
        """The layout loop of this scene graph as a model file for hosts without Python (es_model_load + es_layout_sample).
        ``keep=True``: the masked loop (es_layout_sample_keep); the file also names the regions "x0" [O, 8], "mask" [O], "knoise"
        [T, O * 8] and "ktab" [T, 2]."""
        from .plan import save_model
        st = self._plan_for(obj_embed, triples, keep=keep)
        # (a 'ddim' denoiser's plan ends in es_ddim_rows_update: es_layout_sample / es_layout_sample_keep replay it the same way,
        #  with n_iter for T)
        regions = dict(x=st['x'], noise=st['noise'], step=st['step'], coef=self.coef)
        if keep:
            regions.update(x0=st['x0'], mask=st['mask'], knoise=st['knoise'], ktab=self.keep_tab)
        return save_model(st['plan'], path, regions)

    def eps(self, x, obj_embed, triples, iteration):
        """One UNet1DModel.forward at loop iteration ``iteration`` (t = T-1-iteration)."""
        st = self._plan_for(obj_embed, triples)
        st['x'].copy_(x.to(self.device))
        st['eps_plan'].sample(st['step'], int(iteration), 1, use_graph=False)
        torch.cuda.synchronize()
        return st['eps'].value()

    def _fill_keep(self, st, x0, mask, keep_noise):
        """inputs of the masked loop into the plan's buffers (validation as ShapeDenoiser._fill_keep)"""
        O, D = st['x'].shape
        x0, mask = _check_mask(x0, mask, (O, D), 'masked layout loop', '[O, %d]' % D, 'node')
        n = self.n_iter
        if keep_noise is not None and (keep_noise.dim() < 2 or keep_noise.shape[0] < n or keep_noise[0].numel() != O * D):
            raise ValueError('masked layout loop: keep_noise must be [T, O, %d] with T = %d' % (D, n))
        st['x0'].copy_(x0.to(self.device).float())
        st['mask'].copy_(mask.to(self.device))
        if keep_noise is None:
            st['knoise'].normal_()
        else:
            st['knoise'].copy_(keep_noise.to(self.device).float()[:n].reshape(n, O * D))

    def _prime_keep(self, st):
        """kept rows of x_T <- q_sample(x0, t of iteration 0 -- of this denoiser's schedule --, keep_noise[0]): the one launch in front of the masked loop
        (es_ddim_blend does exactly this arithmetic at n = 8); every later q_sample is written by the step's update launch"""
        O, D = st['x'].shape
        a = hip.BlendArgs()
        a.x, a.x0, a.mask, a.noise = st['x'].data_ptr(), st['x0'].data_ptr(), st['mask'].data_ptr(), st['knoise'].data_ptr()
        a.noise_stride, a.tab, a.step, a.O, a.n = O * D, self.keep_tab.data_ptr(), st['step'].data_ptr(), O, D
        st['step'].zero_()
        import ctypes
        hip.check(hip.lib().es_ddim_blend(ctypes.byref(a), hip.current_stream()), 'es_ddim_blend')

    def stage(self, obj_embed, triples, noise=None, x0=None, mask=None, keep_noise=None, clip=False, prime=True):
        """One call's inputs into its plan state, which is returned ready to run.  The device draws happen in THIS order (a contract:
        a caller who seeds the generator gets the same bits from the same draws made by hand): the keep table [T, O * 8], then
        ``noise`` [T + 1, O, 8] (T = ``n_iter``: the schedule's length under 'ddim', whatever eta is).  ``prime``: the launch that forward-noises the kept rows of x_T (not for a run of no steps)."""
        _check_keep_pair(x0, mask, keep_noise, 'the masked layout loop')
        st = self._plan_for(obj_embed, triples, clip=clip, keep=mask is not None)
        if mask is not None:
            self._fill_keep(st, x0, mask, keep_noise)
        if noise is None:
            st['noise'].normal_()
        else:
            st['noise'][:noise.shape[0]].copy_(noise.to(self.device))
        st['x'].copy_(st['noise'][0])
        if mask is not None and prime:
            self._prime_keep(st)
        return st

    def sample(self, obj_embed, triples, noise=None, n_steps=None, use_graph=True, clip_denoised=False, x0=None, mask=None,
               keep_noise=None):
        """p_sample_loop_sg: returns x_0 [O, 8].  ``noise`` f32[T+1, O, 8] (row 0 = x_T, row 1+i = draw of
        iteration i) makes the run reproducible against the CPU oracle; None draws it on the device.
        ``clip_denoised``: clamp the predicted x0 to [-1, 1] in every step (diffusion_ddpm.py:243-244; the shipped call passes False).

        Masked loop -- keep given boxes while the others are placed around them: ``mask`` [O] with 1 = keep, 0 = generate, ``x0`` f32
        [O, 8] the kept nodes' rows in the model's normalised space (rows with mask 0 are not read) and ``keep_noise`` f32 [T, O, 8]
        the draws of q_sample, row i for iteration i (None: drawn on the device).  Before the denoiser of iteration i (t = T-1-i) the
        kept rows are ``sqrt_ac[t] * x0 + sqrt(1 - ac)[t] * keep_noise[i]`` (GaussianDiffusion.q_sample, diffusion_ddpm.py:191-201; the
        reference defines the masked loop for shapes only, samplers/ddim.py:160-163); they take part in the step's message passing
        like every other node; after the last iteration they are ``x0`` bit for bit.  A run stopped early (``n_steps`` < T) leaves
        them at the NEXT timestep's forward-noised value.  ``clip_denoised`` never touches kept rows.  ``mask=None``: the loop and
        its plan are what they are without this feature.

        A ``sampler='ddim'`` denoiser runs DDIMSampler.ddim_sampling on its strided schedule instead: T above reads ``n_iter`` (the
        schedule's length), iteration i is at timestep ``sched.timesteps[i]``, row 1 + i of ``noise`` is the randn draw that sigma_i
        scales (read only when eta != 0; the table keeps its [n_iter + 1, O, 8] form either way), the masked loop blends with
        q_sample at those timesteps, and ``clip_denoised=True`` is refused."""
        if self.sampler == 'ddim' and clip_denoised:
            raise ValueError('layout DDIM: clip_denoised=True has no reference arithmetic under DDIM (p_sample_ddim never clips)')
        n_steps = self.n_iter if n_steps is None else n_steps
        if not 0 <= n_steps <= self.n_iter:
            raise ValueError('n_steps must be in [0, %d] (the iterations of the schedule), got %r' % (self.n_iter, n_steps))
        st = self.stage(obj_embed, triples, noise, x0, mask, keep_noise, clip=bool(clip_denoised), prime=n_steps > 0)
        st['plan'].sample(st['step'], 0, n_steps, use_graph=use_graph)
        return st['x'].clone()


CANON_OBJECTS = 4      # objects of the reference shard of ShapeDenoiser(deterministic=True): 32 objects over the 8 GPUs of one node


class ShapeDenoiser:
    """UNet3DModel + DDIM sampling on the HIP path (loop B of SURVEY.md section 3.1):
    ``EchoToShape.rel2shape`` without the VQ-VAE decode (echo2shape.py:484-521).

    ``rank`` / ``world``: object sharding over GPUs (echoscene_amd/parallel.py).  world == 1 runs the whole
    step as one hipGraph; world > 1 splits each step at the echo all-gather."""

    def __init__(self, df, model_params=None, ddim_steps=100, device=None, z_shape=(3, 16, 16, 16), rank=0, world=1,
                 group=None, deterministic=False, force_exchange=False, precision='fp16', ddim_eta=0.0, sampler='ddim', weights=None,
                 up_fold=True):
        """``force_exchange``: build the sharded step structure (stem plan -> code exchange -> main plan) even at world == 1 --
        the one-GPU test of the captured RCCL exchange (tests/test_hip_scene.py).
        ``precision``: 'fp16' (product: fp16 MFMA operands, fp32 accumulate) or 'fp32' -- the VALIDATION route: fp32 activations and
        weights on the exact-fp32 matrix instruction (csrc/es_vol32.hip, 1/16 of the fp16 matrix rate), i.e. the reference's own
        arithmetic (openai_model_3d.py:816-863 is fp32 everywhere), so that the cost of operand rounding is a measurement."""
        # ``ddim_eta`` != 0: stochastic DDIM -- every step adds sigma_t * randn (samplers/ddim.py:256-260); the draws of a run are a
        # device table [S, objects x latent] filled per sample() (or handed in: ``step_noise``)
        # 'fp32x' (round 6): fp32 activations, fp32 attention / norms, and every contraction on the f16 matrix pipe with SPLIT operands
        # (x = hi + lo in f16, three partial products accumulated in fp32: plan_vol.PackedConvX3) -- the reference's arithmetic to
        # ~2^-21 per product at 3x the K of the product route, instead of the 1/16 matrix rate of 'fp32'
        # ``sampler``: 'ddim' (the shipped loop) or 'plms' -- the reference's PLMSSampler (samplers/plms.py) on the SAME schedule and
        # tables: pseudo linear multistep, S + 1 denoiser evaluations for S iterations (schedules.plms_evaluations), the usual way to halve
        # the step count of a deterministic sampler.  ``sample(sampler=)`` may override it per call (each sampler has plans of its own).
        # ``weights``: the packed UNet3DWeights of another ShapeDenoiser of the same network, device and precision (another step count or
        # sampler does not need a second copy of them)
        if precision not in ('fp16', 'fp32', 'fp32x'):
            raise ValueError("precision must be 'fp16', 'fp32' or 'fp32x'")
        if sampler not in SHAPE_SAMPLERS:
            raise ValueError('sampler must be one of %s, got %r' % (SHAPE_SAMPLERS, sampler))
        self.sampler = sampler
        self.precision = precision
        self.force_exchange = bool(force_exchange)
        self.device = device or torch.device('cuda')
        self.df = df
        net = df.diffusion_net
        self.net = net
        if weights is not None:
            if getattr(weights, 'precision', None) != precision:
                raise ValueError('weights were packed for precision %r, this denoiser asks for %r' % (getattr(weights, 'precision', None), precision))
            self.w = weights
        else:
            sd = {k[len('diffusion_net.'):]: v for k, v in state_dict_for(df, self.device).items()}
            self.w = UNet3DWeights(sd, net, self.device, precision)
        mp = dict(model_params or {})
        self.ddim_eta = float(ddim_eta)
        self.sched = ShapeSchedule(ddim_steps, mp.get('timesteps', 1000), mp.get('linear_start', 0.00085),
                                   mp.get('linear_end', 0.012), eta=self.ddim_eta)
        self.S = len(self.sched.timesteps)
        if sampler == 'plms':
            self._check_plms()
        self.z_shape = tuple(z_shape)
        self.per = math.prod(int(d) for d in self.z_shape)       # elements of one object's latent
        self.temb = timestep_embedding_table(self.sched.timesteps, net.model_channels).to(self.device)
        self.coef = self.sched.coef.to(self.device)
        self.keep_tab = self.sched.keep_tab.to(self.device)      # masked DDIM: q_sample's factors per iteration (es_ddim_blend)
        self.rank, self.world, self.group = rank, world, group
        # deterministic=True ("the 8-GPU result must equal the 1-GPU result bit for bit"): the CANONICAL
        # arithmetic -- every K split and partial-sum tiling is a function of the layer alone: the one a reference shard of
        # CANON_OBJECTS objects takes (es_conv_args.O_hint < 0), on every rank of every world size, 1 included.  All world sizes
        # then produce the same bits, and the shard sizes of the 8-GPU partition are the fast ones.  (Rounds 4-5 took the unsharded
        # run's splits as the canon: its small shards then ran K chains tuned for 8x their rows -- x1.9 at 8 GPUs.)  The price
        # is paid where it hurts least: a canonical run with MORE objects per GPU than the reference splits K more than it needs.
        # deterministic=False (the default since round 6): every rank tunes its splits to its own share; results differ between
        # world sizes in fp32 summation order only (5e-4 relative after 4 steps, inside the 2e-2 parity budget).  At 4 objects
        # per GPU the two modes are the same arithmetic.
        self.deterministic = deterministic
        # ``up_fold`` (default on): the two up-sampling convs of the step carry their folded weight image (plan_vol.up_fold_weights:
        # 12 taps per parity class instead of 27) and the library multiplies through it where the launch is eligible.  False: the
        # plan omits the image -- the 27-tap arithmetic, for A/B runs and bisecting without a rebuild.  Never with deterministic=True.
        self.up_fold = bool(up_fold)
        self.tables = time_tables(self.w, self.temb, self.w.shape_t, self.device)
        self._plans, self.max_plans = {}, 2
        self._cur, self._use_graph = None, True                  # the state / graph switch the shard protocol below works on
        # the fused (layout + shape) graph of sample_layout_and_shape, built on one of the resident plans (fused_plan)
        self._fused, self._fused_key = None, None

    def _check_plms(self):
        """PLMS needs eta = 0 (PLMSSampler.make_schedule raises the same way, plms.py:28-29) and two timesteps: with one, the reference
        evaluates the denoiser twice at the same t (t_next = t, plms.py:152); that degenerate run is not offered."""
        if self.ddim_eta != 0.0:
            raise ValueError('ddim_eta must be 0 for PLMS')
        if self.S < 2:
            raise ValueError('PLMS needs at least 2 timesteps (ddim_steps=%d yields %d)' % (self.S, self.S))

    def _sampler_of(self, sampler):
        sampler = self.sampler if sampler is None else sampler
        if sampler not in SHAPE_SAMPLERS:
            raise ValueError('sampler must be one of %s, got %r' % (SHAPE_SAMPLERS, sampler))
        if sampler == 'plms':
            self._check_plms()
        return sampler

    def _insert_plan(self, key, st):
        """bounded plan cache: evicting a plan also drops the fused (layout + shape) graph built on it -- each resident plan
        owns its activation buffers, split-K workspace and captured graph (several GB at O = 32)"""
        while len(self._plans) >= self.max_plans:
            old = self._plans.pop(next(iter(self._plans)))
            if self._fused_key is not None and old['plan'] is not None and self._fused_key[1] == id(old['plan']):
                self._fused, self._fused_key = None, None
        self._plans[key] = st

    def fused_plan(self, layout_plan, ss, r):
        """the plan of one shape step of the state ``ss`` with ``r`` steps of ``layout_plan`` on a parallel branch (plan.combine_plans).
        One per denoiser: a caller that alternates ``shape_sampler`` per call on ONE denoiser re-captures it every call; the scene layer
        keeps a denoiser per sampler, so each has its own."""
        from .plan import combine_plans
        key = (id(layout_plan), id(ss['plan']), r)
        if self._fused_key != key:
            self._fused, self._fused_key = combine_plans(self.device, ss['plan'], layout_plan, side_repeat=r), key
        return self._fused

    def _build_state(self, uc, triples, c, O, cap, keep, sampler, sig):
        """a cache miss: emit the step for this rank's objects, compose its sub-plans"""
        from .parallel import partition
        lo, hi, block = partition(O, self.world, self.rank)
        if hi == lo:
            # more ranks than object blocks: this rank owns nothing.  It runs no kernels but keeps joining the
            # collectives of the loop (a rank that raised here would leave the others blocked in the all-gather).
            z = lambda *sh: torch.zeros(*sh, device=self.device)
            return new_state(empty=True, x=z(0, *self.z_shape), eps=z(0, *self.z_shape), lo=lo, hi=hi, O=O, codes_local=z(block, 64),
                             codes_all=z(block * self.world, 64), sig=sig, sampler=sampler)
        g = GraphIndex(triples, O, self.device, capacity=cap)
        # deterministic: split-K / partial-sum tiling of the reference shard -> bit-identical latents at every world size
        b = Builder(self.device, precision=self.precision, o_hint=-CANON_OBJECTS if self.deterministic else 0,
                    up_fold=self.up_fold and not self.deterministic, shard_block=block, force_exchange=self.force_exchange)
        plms = sampler == 'plms'
        bufs = emit_shape_step(b, self.w, g, uc, self.temb, self.tables, self.coef, self.keep_tab, self.S, self.z_shape, lo, hi,
                               c_local=None if c is None else c[lo:hi], gather_rows=block * self.world, keep=bool(keep), plms=plms,
                               step_noise=self.ddim_eta != 0.0, keep_vox=keep == 'vox')
        ops = compose_step_plans(b.ops, bufs.pop('n_blend'), bufs.pop('split'), bufs.pop('n_eps_ops'), *bufs.pop('first_ops'), plms=plms,
                                 sharded=(self.world > 1 or self.force_exchange) and self.w.mp)
        st = new_state(lo=lo, hi=hi, O=O, g=g, sig=sig, sampler=sampler, **bufs)
        made = {id(ops['plan']): b.finish()}                     # (the step itself owns the scratch claim; the others are views of it)
        for name in SUB_PLANS:
            if ops[name] is not None:
                if id(ops[name]) not in made:
                    made[id(ops[name])] = sub_plan(b, ops[name])
                st[name] = made[id(ops[name])]
        return st

    def _plan_for(self, uc, triples, c=None, keep=False, sampler=None):
        """``sampler='plms'``: the plans of the PLMS loop, under a cache key of their own -- 'plan' is the steady iteration (the denoiser
        ops, then es_plms_update in the place of es_ddim_update) and 'first_plan' iteration 0 (the denoiser ops, es_plms_first_a, the
        denoiser ops again, es_plms_first_b); the blend of ``keep=True`` sits in front of the FIRST evaluation only (the reference blends
        once per iteration, before p_sample_plms, plms.py:154-159).  The 'ddim' plans are, op for op, what they have always been.
        ``keep=True``: the plan of the MASKED loop -- one more op, the blend (es_ddim_blend), in front of the step's denoiser ops,
        and its three inputs: ``x0`` [Ol, C,D,H,W], ``mask`` [Ol], ``knoise`` [S, Ol * latent].  A plan of its own (another cache key):
        without a mask the plan is, op for op, what it has always been.
        ``keep='vox'``: the voxel form of the masked loop (shape completion) -- the same plan with es_ddim_blend_vox for the blend and
        ``mask`` [Ol, D * H * W]; again a cache key of its own ('keepvox'), so the two plans above stay what they are."""
        uc = uc.reshape(uc.shape[0], -1)
        O = uc.shape[0]
        concat = self.w.concat
        if concat or not self.w.mp:             # c_s is unused only by 'crossattn' WITH message passing
            if c is None:
                raise ValueError("this shape denoiser needs the conditioning c_s (concat: [O, 4096], echo2shape.py:234-235; "
                                 "no message passing: the cross-attention key [O, 1, context_dim])")
            c = c.reshape(O, -1).to(self.device).float()
        else:
            c = None
        cap = _cap(triples.shape[0])
        sampler = self._sampler_of(sampler)
        key = ((O, cap, 'keepvox' if keep == 'vox' else 'keep') if keep else (O, cap)) + (('plms',) if sampler == 'plms' else ())
        sig = hash(triples.detach().cpu().numpy().tobytes())
        st = self._plans.get(key)
        if st is None:
            st = self._build_state(uc, triples, c, O, cap, keep, sampler, sig)
            self._insert_plan(key, st)
        elif st['sig'] != sig and not st['empty']:
            # same size class, another scene graph: rewrite indices / predicate rows in place, keep plans and graphs
            st['g'].update(triples)
            if st['pred'] is not None:
                st['pred'].copy_(self.w.pred_table[torch.from_numpy(st['g'].p_host)])
            st['sig'] = sig
        if st['empty']:
            return st
        if st['objbuf'] is not None:
            st['objbuf'][:, :st['ucw']].copy_(uc.to(self.device))
        if concat:
            st['xc'][:, 3].copy_(c[st['lo']:st['hi']])
        elif st['cdev'] is not None:
            st['cdev'].copy_(c[st['lo']:st['hi']])
        return st

    # -- shard backend protocol of parallel.sharded_ddim_loop ------------------------------------------------
    def passes(self, i):
        """(stem -> exchange -> rest) passes of loop iteration i: 2 in iteration 0 of a PLMS loop (its second evaluation), else 1"""
        return 2 if (self._cur['sampler'] == 'plms' and int(i) == 0) else 1

    def codes_local(self, i, p=0):
        st = self._cur
        if not st['empty']:
            # pass 1 (PLMS iteration 0): the stem without the blend, at the step counter first-a left (1: the reference's t_next)
            plan, first = (st['stem2_plan'], 1) if p else (st['stem_plan'], int(i))
            plan.sample(st['step'], first, 1, use_graph=self._use_graph)     # captured like the main part
        return st['codes_local']

    def gather_buffers(self):
        """(send block [block, 64], receive buffer [world * block, 64]) of the per-step echo all-gather: pre-allocated, the
        stem plan writes the first, the main plan's first op reads the second."""
        st = self._cur
        return st['codes_local'], st['codes_all']

    def step(self, i, codes_all, p=0):
        st = self._cur
        if st['empty']:
            return
        if codes_all.data_ptr() != st['codes_all'].data_ptr():      # single-process emulations hand in their own tensor
            st['codes_all'][:codes_all.shape[0]].copy_(codes_all)
        plan, first = st['main_plan'], int(i)
        if st['sampler'] == 'plms' and int(i) == 0:
            plan, first = (st['main_b_plan'], 1) if p else (st['main_a_plan'], 0)
        plan.sample(st['step'], first, 1, use_graph=self._use_graph)

    def latents_local(self):
        return self._cur['x']

    def save_model(self, path, uc, triples, c=None, keep=False):
        """The DDIM loop of this scene (single GPU) as a model file for hosts without Python (es_model_load + es_shape_sample).
        ``keep=True``: the masked loop; the host fills the regions "x0" [O,C,D,H,W], "mask" [O] and "keep_noise" [S, O x latent].
        ``keep='vox'``: the voxel form of the masked loop (shape completion); the region "mask" is then O * V floats, one per latent
        voxel ([O, D * H * W]), filled by the host in the same way."""
        from .plan import save_model
        if self.sampler == 'plms':
            raise NotImplementedError("model files hold the DDIM loop only (es_shape_sample); sampler='plms' has no C host yet")
        assert self.world == 1 and not self.force_exchange
        st = self._plan_for(uc, triples, c, keep=keep)
        regions = dict(x=st['x'], step=st['step'], coef=self.coef)
        if keep:
            regions.update(x0=st['x0'], mask=st['mask'], keep_noise=st['knoise'])
        if st['snoise'] is not None:
            # ddim_eta != 0: the per-step draws [S, objects x latent] are an INPUT of the loop -- a named region the host fills before
            # es_shape_sample (es_model_region(m, "step_noise")); the file stores whatever the table holds now
            regions['step_noise'] = st['snoise']
        return save_model(st['plan'], path, regions)

    def step_graph(self, group=None):
        """ONE graph per DDIM step of the sharded loop ("RCCL on a dedicated stream, or direct peer
        writes for the 8 KB"): this rank's stem ops -> the RCCL all-gather of the [block, 64] codes -> everything else, captured
        together (torch.cuda.CUDAGraph: ProcessGroupNCCL collectives are capturable), so a step is a single graph launch with no
        host round trip between its three parts.  The step counter lives on the device and is advanced by the captured DDIM
        update.

        OPT-IN (``ES_STEP_GRAPH=1``): the captured exchange has only ever run on a 1-rank NCCL group (one GPU per box here), so
        the default is the three-call step (graph launch / collective / graph launch), which the 2-rank tests do cover.  When it
        is enabled the graph-or-eager decision is COLLECTIVE: every rank attempts the capture, then all ranks all-reduce (MIN) a
        success flag and ALL fall back to the three-call step if any rank failed -- a rank must never replay captured all-gathers
        while a peer issues eager ones after a failed capture.  A rank without objects captures nothing and issues
        one eager all-gather per step; that matches its peers' captured ones call for call.
        Returns the graph, or None (three-call step)."""
        st = self._cur
        if st['sampler'] == 'plms':
            return None                          # the captured step graph is the DDIM step; PLMS runs the three-call step
        if not self._use_graph or (st['stem_plan'] is None and not st['empty']) or os.environ.get('ES_STEP_GRAPH', '0') != '1':
            return None
        if 'step_graph' in st:
            return st['step_graph']
        st['step_graph'] = None
        import torch.distributed as dist
        if not dist.is_initialized() or dist.get_backend(group) != 'nccl':
            return None                          # (decided from the backend alone: the same on every rank)
        send, recv = st['codes_local'], st['codes_all']
        g, ok = None, 1
        # communicator set-up outside any capture; every rank (an empty shard too) takes part (recv is scratch)
        dist.all_gather_into_tensor(recv, send, group=group)
        torch.cuda.synchronize(self.device)
        if not st['empty']:
            try:
                s = torch.cuda.Stream(device=self.device)
                s.wait_stream(torch.cuda.current_stream(self.device))
                with torch.cuda.stream(s):
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g, stream=s):
                        st['stem_plan'].run()
                        dist.all_gather_into_tensor(recv, send, group=group)
                        st['main_plan'].run()
                torch.cuda.current_stream(self.device).wait_stream(s)
            except Exception as e:                 # noqa: BLE001 -- any capture problem on this rank
                import warnings
                warnings.warn('sharded DDIM step: the RCCL exchange could not be captured on rank %d (%s)' % (self.rank, e))
                g, ok = None, 0
        flag = torch.tensor([ok], dtype=torch.int32, device=self.device)
        dist.all_reduce(flag, op=dist.ReduceOp.MIN, group=group)      # collective decision: all ranks replay, or none does
        if int(flag.item()) != 1:
            g = None
        st['step_graph'] = g
        return g

    def begin(self, first_step):
        """set the device step counter (the captured step graph does not re-set it every replay)"""
        self._cur['step'].fill_(int(first_step))

    def eps(self, x, uc, triples, iteration, c=None):
        assert self.world == 1
        st = self._plan_for(uc, triples, c)
        st['x'].copy_(x.to(self.device))
        st['eps_plan'].sample(st['step'], int(iteration), 1, use_graph=False)
        return st['eps'].clone()

    @staticmethod
    def _run_loop(st, n_steps, use_graph):
        """the unsharded loop of a plan state: DDIM replays 'plan'; PLMS runs iteration 0 ('first_plan': two evaluations, the step
        counter ends at 1) and replays the steady 'plan' for the others"""
        if st['sampler'] == 'plms':
            if n_steps > 0:
                st['first_plan'].sample(st['step'], 0, 1, use_graph=use_graph)
                st['plan'].sample(st['step'], 1, n_steps - 1, use_graph=use_graph)
        else:
            st['plan'].sample(st['step'], 0, n_steps, use_graph=use_graph)

    def _fill_table(self, st, name, given):
        """this rank's objects lo:hi of a per-step, per-object table [S, O, latent] into the buffer ``st[name]`` [S, (hi - lo) * latent]:
        ``given`` by the caller, or drawn on the device.  Sharded, the table of the WHOLE scene is drawn on every rank -- also one that
        owns no object (more ranks than objects) -- and sliced: ranks seeded alike (as they must be for noise1) draw what the
        unsharded run draws and stay in step; a rank that skipped the draw left its generator behind the others' (ADVICE r5).  ONE
        randn call, as the unsharded run's normal_(): a chunked draw is another Philox stream (transient: S * O * latent floats)."""
        O, lo, hi = st['O'], st['lo'], st['hi']
        if given is None and self.world > 1:
            given = torch.randn(self.S, O, self.per, device=self.device)
        if st['empty']:
            return
        if given is None:
            st[name].normal_()
        else:
            t = given.to(self.device).float().reshape(given.shape[0], O, self.per)[:self.S, lo:hi]
            st[name][:t.shape[0]].copy_(t.reshape(t.shape[0], -1))

    def _fill_keep(self, st, x0, mask, keep_noise):
        """inputs of the masked loop into the plan's buffers (this rank's objects lo:hi of the scene's)"""
        O, lo, hi = st['O'], st['lo'], st['hi']
        x0, mask, _ = _check_shape_mask(x0, mask, O, self.z_shape)         # (per object [O] or per voxel [O, V]: rows lo:hi either way)
        if keep_noise is not None and (keep_noise.shape[0] < self.S or keep_noise[0].numel() != O * self.per):
            raise ValueError('masked DDIM: keep_noise must be [S, O, C, D, H, W]')
        if not st['empty']:
            st['x0'].copy_(x0.to(self.device).float()[lo:hi])
            st['mask'].copy_(mask.to(self.device)[lo:hi])
        self._fill_table(st, 'knoise', keep_noise)

    def stage(self, uc, triples, c=None, noise1=None, step_noise=None, x0=None, mask=None, keep_noise=None, sampler=None):
        """One call's inputs into its plan state, which is returned ready to run.  The device draws happen in THIS order (a contract:
        ranks seeded alike stay in step, and a caller who seeds the generator gets the same bits from the same draws made by hand):
        the keep table [S, O * latent], then ``noise1`` [1, C, D, H, W], then ``step_noise`` [S, O * latent] (eta != 0 only); sharded, the
        two tables are those of the whole scene on every rank (_fill_table)."""
        _check_keep_pair(x0, mask, keep_noise, 'masked DDIM')
        keep = False
        if mask is not None:
            x0, mask, vox = _check_shape_mask(x0, mask, uc.shape[0], self.z_shape)
            keep = 'vox' if vox else True
        st = self._plan_for(uc, triples, c, keep=keep, sampler=sampler)
        if mask is not None:
            self._fill_keep(st, x0, mask, keep_noise)
        if noise1 is None:
            noise1 = torch.randn((1,) + self.z_shape, device=self.device)
        st['x'].copy_(noise1.to(self.device).expand(st['hi'] - st['lo'], *self.z_shape))
        if self.ddim_eta != 0.0:
            self._fill_table(st, 'snoise', step_noise)
        return st

    def sample(self, uc, triples, noise1=None, n_steps=None, use_graph=True, c=None, step_noise=None, x0=None, mask=None,
               keep_noise=None, sampler=None):
        """DDIM loop; ``noise1`` f32[1,C,D,H,W] is shared by all objects as in the reference
        (echo2shape.py:507-510); None draws it on the device (world > 1: pass it, or every rank draws its own).
        ``step_noise`` (ddim_eta != 0 only) f32[S, O, C,D,H,W]: the per-step draws of p_sample_ddim, one per OBJECT (noise_like without
        repeat, ldm_diffusion_util.py:289-292); None draws them on the device.

        Masked DDIM (``DDIMSampler.sample(mask=, x0=)``, samplers/ddim.py:160-163) -- keep given shapes while the others are
        generated: ``mask`` [O] with 1 = keep, 0 = generate, ``x0`` f32[O,C,D,H,W] the kept objects' latents (rows with mask 0 are not
        read; ``VQEncoder.encode_no_quant`` of their SDFs) and ``keep_noise`` f32[S,O,C,D,H,W] the draws of q_sample (None: drawn on the
        device).  Before every step the kept rows are set to ``sqrt_ac[t] * x0 + sqrt(1 - ac)[t] * keep_noise[step]``; they take part
        in the step's echo message passing like every other node.  ``mask=None``: the loop and its plan are what they are without this
        feature.
        Shape completion (``shape_comp``, diffusion_shape/sdfusion_model.py:400-446): ``mask`` may also be per latent VOXEL --
        [O, 1, D, H, W] or [O, D, H, W] of zeros and ones, one value for the C channels, the ``z_mask`` of get_partial_shape
        (postprocess.latent_range_mask) -- with ``x0`` the encoding of the WHOLE given shape: the voxels with mask 1 follow the
        forward-noised trajectory of ``x0``, the others are generated (es_ddim_blend_vox; a plan of its own).  An all-ones row is a
        kept object, bit for bit the per-object loop's; an all-zero row a generated one.  The reference accepts any tensor as mask;
        these two forms are offered, and any other shape -- a mask per channel [O, C, D, H, W] too -- is a ValueError.
        ``sampler``: 'ddim' / 'plms' for this call (None: the denoiser's own).  PLMS: ``n_steps`` counts ITERATIONS -- iteration 0
        evaluates the denoiser twice (improved Euler), so k iterations are k + 1 evaluations; the masked loop blends once per iteration,
        before its first evaluation.
        Returns the latents of ALL objects [O,C,D,H,W] (all-gathered when sharded)."""
        from .parallel import all_gather_rows, sharded_ddim_loop
        st = self.stage(uc, triples, c, noise1, step_noise, x0, mask, keep_noise, sampler)
        n_steps = self.S if n_steps is None else n_steps
        if not self.w.mp or (self.world == 1 and not self.force_exchange):
            # no exchange inside the loop: each rank runs its own objects (no message passing: ranks only meet at the end)
            if not st['empty']:
                self._run_loop(st, n_steps, use_graph)
            z = st['x'] if self.world == 1 else all_gather_rows(st['x'], st['O'], self.world, self.group)
        else:
            self._cur, self._use_graph = st, use_graph
            z = sharded_ddim_loop(self, st['O'], n_steps, self.world, self.group)
        return z.clone()


def keep_selection(keep_nodes, n_objects):
    """``keep_nodes`` (indices into the decoder-side node list) -> (mask f32 [O] with 1 = keep, rows: the kept nodes in ascending
    order, src: for each of them the row of ``keep_sdfs`` it takes).  Duplicates and out-of-range entries follow the
    ``manipulated_nodes`` convention (the reference's ``i in list`` tests): a node counts once -- its first entry names its SDF --
    and an entry outside [0, O) is ignored."""
    first = {}
    for k, t in enumerate(keep_nodes):
        t = int(t)
        if 0 <= t < n_objects and t not in first:
            first[t] = k
    rows = sorted(first)
    mask = torch.zeros(n_objects, dtype=torch.float32)
    if rows:
        mask[rows] = 1.0
    return mask, rows, [first[t] for t in rows]


def fused_iterations(n_iter_layout, n_iter_shape, first=0):
    """Iteration arithmetic of the fused call: (r, left) = the layout steps on the parallel branch of every fused replay and the layout
    steps that run afterwards.  The fused graph replays for the shape iterations ``first`` .. S-1 (``first`` = 1 under PLMS, whose
    iteration 0 runs unfused); r = 0 (fewer layout than shape iterations): nothing is fused and the whole layout loop is left."""
    r = int(n_iter_layout) // int(n_iter_shape)
    done = r * (int(n_iter_shape) - int(first)) if r >= 1 else 0
    return r, int(n_iter_layout) - done


def sample_layout_and_shape(lay, shp, obj_embed, triples, uc, c=None, layout_noise=None, shape_noise=None, use_graph=True,
                            x0=None, mask=None, keep_noise=None, box_x0=None, box_mask=None, box_keep_noise=None, shape_sampler=None):
    """Both sampling loops of one scene (EchoScene.py:402-419 runs them back to back) as ONE replayed hipGraph: every replay = one
    shape step on the main branch and ``r = n_iter_layout // n_iter_shape`` (= 10 by default) layout steps on a parallel branch
    (plan.combine_plans).  The parallel branch does NOT hide the latency-bound layout chain: measured end to end
    (profiles/r06_e2e_latency.txt) a scene call costs the plain sum of its two loops, the 1000-step layout loop 0.65 s of it at
    any scene size -- which is why a shorter layout loop (``LayoutDenoiser(sampler='ddim', steps=...)``) shortens the call.
    Left-over layout steps (n_iter_layout not a multiple of the shape iterations) run afterwards; r = 0 (fewer layout than shape
    iterations) runs the two loops unfused.  Returns (boxes x_0 [O, 8], latents z_0).
    ``x0`` / ``mask`` / ``keep_noise``: the masked shape loop (ShapeDenoiser.sample).  ``box_x0`` / ``box_mask`` / ``box_keep_noise``:
    the masked layout loop (LayoutDenoiser.sample) -- its keep plan is then the side branch of the fused graph and runs the left-over
    steps; the two families are independent of each other.
    ``shape_sampler``: 'ddim' / 'plms' for the shape loop (None: the denoiser's own).  PLMS: iteration 0 (two evaluations) runs unfused,
    iterations 1..S-1 replay the fused graph, and the layout steps not covered run afterwards.
    Inputs are staged layout first, then shape (LayoutDenoiser.stage, ShapeDenoiser.stage: the order of the device draws); a
    ``ddim_eta`` != 0 shape denoiser draws its step-noise table last (this call has no argument to pass that table in)."""
    _check_keep_pair(box_x0, box_mask, box_keep_noise, 'the masked layout loop', 'box_')
    if shp.world != 1:
        return lay.sample(obj_embed, triples, noise=layout_noise, use_graph=use_graph, x0=box_x0, mask=box_mask,
                          keep_noise=box_keep_noise), \
            shp.sample(uc, triples, noise1=shape_noise, c=c, use_graph=use_graph, x0=x0, mask=mask, keep_noise=keep_noise,
                       sampler=shape_sampler)
    st = lay.stage(obj_embed, triples, layout_noise, box_x0, box_mask, box_keep_noise)
    ss = shp.stage(uc, triples, c, shape_noise, None, x0, mask, keep_noise, shape_sampler)
    first = 1 if ss['sampler'] == 'plms' else 0                 # PLMS: iteration 0 is not a replay of the steady step
    r, _ = fused_iterations(lay.n_iter, shp.S, first)
    done = 0
    if r >= 1 and use_graph:
        fused = shp.fused_plan(st['plan'], ss, r)
        st['step'].zero_()
        if first:
            ss['first_plan'].sample(ss['step'], 0, 1, use_graph=True)
        fused.sample(ss['step'], first, shp.S - first, use_graph=True)
        done = r * (shp.S - first)
    else:
        shp._run_loop(ss, shp.S, use_graph)
    if done < lay.n_iter:
        st['plan'].sample(st['step'], done, lay.n_iter - done, use_graph=use_graph)
    return st['x'].clone(), ss['x'].clone()


def _run_chunks(codec, src, out, dims, src_key, dst_key, sync):
    """the chunk loop of VQDecoder / VQEncoder: ``codec.chunk`` objects of ``src`` at a time through the plan of that many objects
    (its input buffer ``src_key``, its result ``dst_key``) into ``out``"""
    for i in range(0, src.shape[0], codec.chunk):
        n = min(codec.chunk, src.shape[0] - i)
        st = codec._plan(n, dims)
        st[src_key].copy_(src[i:i + n])
        st['plan'].run()
        out[i:i + n].copy_(st[dst_key])
    if sync:
        torch.cuda.synchronize()
    return out


class VQDecoder:
    """VQVAE.decode_no_quant on the HIP path: latents [O,3,16,16,16] -> SDF [O,1,64,64,64]
    (the once-per-sample epilogue of rel2shape, echo2shape.py:522).  Objects are decoded in chunks so
    that the 64^3-resolution activations stay bounded."""

    def __init__(self, vqvae, device=None, chunk=8):
        self.device = device or torch.device('cuda')
        self.w = VQWeights(state_dict_for(vqvae, self.device), self.device)
        self.chunk = chunk
        self._plans = {}

    def _plan(self, Oc, zdims):
        key = (Oc, zdims)
        if key not in self._plans:
            b = Builder(self.device)
            z = b.buf(Oc, 3, *zdims)
            od = tuple(4 * d for d in zdims)         # placeholder; real dims come from the emitter
            sdf = b.buf(Oc, 1, *od)
            dm = emit_vq_decode(b, self.w, z, sdf, Oc, zdims)
            assert tuple(dm) == od, (dm, od)
            self._plans = {key: dict(plan=b.finish(), z=z, sdf=sdf)}
        return self._plans[key]

    def save_model(self, path, n_objects, zdims=(16, 16, 16)):
        """The decoder for ``n_objects`` latents as a model file for hosts without Python (es_model_load + es_vq_decode)."""
        from .plan import save_model
        st = self._plan(n_objects, tuple(zdims))
        return save_model(st['plan'], path, dict(z=st['z'], sdf=st['sdf']))

    def decode_no_quant(self, z, sync=True):
        """``sync=False``: everything is only enqueued on the current stream (the caller orders consumers)."""
        z = z.to(self.device).float().contiguous()
        O = z.shape[0]
        zdims = tuple(z.shape[2:])
        n_up = len([1 for _, up in self.w.levels if up is not None])
        out = torch.empty(O, 1, *[d * 2 ** n_up for d in zdims], device=self.device)
        return _run_chunks(self, z, out, zdims, 'z', 'sdf', sync)


class VQEncoder:
    """VQVAE.encode_no_quant on the HIP path (vqvae_networks/network.py:84-88): truncated SDFs [O,1,64,64,64] -> the unquantised latents
    [O,3,16,16,16] the shape denoiser works on -- ``x0`` of the masked DDIM loop (ShapeDenoiser.sample).  Objects are encoded in chunks
    (the 64^3 activations are 67 MB per object and fp32 buffer at 64 channels).  The quantised ``encode`` (code indices) is not
    offered: the loop consumes the unquantised latent, and fp16 operands cannot reproduce an argmin over near-ties."""

    def __init__(self, vqvae, device=None, chunk=8, precision='fp16'):
        if precision != 'fp16':
            raise NotImplementedError("VQEncoder: precision %r (only 'fp16': fp16 MFMA operands, fp32 accumulation)" % (precision,))
        if chunk < 1 or chunk > 8:
            raise ValueError('VQEncoder: chunk must be 1..8 objects (31-bit byte offsets at 64^3 x 64 channels)')
        self.device = device or torch.device('cuda')
        dd = getattr(vqvae, 'ddconfig', None)
        if dd is not None and dd.get('double_z', False):
            raise NotImplementedError('VQEncoder: double_z encoders are not supported')
        self.w = VQEncWeights(state_dict_for(vqvae, self.device), self.device)
        self.chunk = chunk
        self._plans = {}

    def _plan(self, Oc, dims):
        key = (Oc, dims)
        if key not in self._plans:
            b = Builder(self.device)
            sdf = b.buf(Oc, 1, *dims)
            zd = tuple(d >> self.w.n_down for d in dims)
            z = b.buf(Oc, self.w.embed_dim, *zd)
            dm = emit_vq_encode(b, self.w, sdf, z, Oc, dims)
            assert tuple(dm) == zd, (dm, zd)
            self._plans = {key: dict(plan=b.finish(), z=z, sdf=sdf)}
        return self._plans[key]

    def save_model(self, path, n_objects, dims=(64, 64, 64)):
        """The encoder for ``n_objects`` SDFs as a model file for hosts without Python (es_model_load, regions "sdf" -> "z")."""
        from .plan import save_model
        st = self._plan(n_objects, tuple(dims))
        return save_model(st['plan'], path, dict(sdf=st['sdf'], z=st['z']))

    def encode_no_quant(self, sdf, sync=True):
        """``sync=False``: everything is only enqueued on the current stream (the caller orders consumers)."""
        sdf = sdf.to(self.device).float().contiguous()
        if sdf.dim() != 5 or sdf.shape[1] != 1:
            raise ValueError('encode_no_quant: sdf must be [O, 1, D, H, W], got %s' % (tuple(sdf.shape),))
        O = sdf.shape[0]
        dims = tuple(sdf.shape[2:])
        out = torch.empty(O, self.w.embed_dim, *[d >> self.w.n_down for d in dims], device=self.device)
        return _run_chunks(self, sdf, out, dims, 'sdf', 'z', sync)
