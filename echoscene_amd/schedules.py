"""Host-side diffusion schedules and per-step coefficient tables (tiny, computed once).

These are the numbers the reference keeps in ``GaussianDiffusion`` / ``DDIMSampler``; they are
prepared on the host in the reference's own precision order and uploaded as small device tables
that the step plans index with the on-device step counter.

  * layout: ``get_betas`` (every schedule type the reference can build) + ``GaussianDiffusion.__init__`` and the
    mean / variance parameterisations of ``p_mean_variance``
    (model/networks/diffusion_layout/diffusion_ddpm.py:38-84, 133-162, 220-264)
  * shape : ``make_beta_schedule('linear')``, ``make_ddim_timesteps('uniform')``,
    ``make_ddim_sampling_parameters`` (diffusion_shape/ldm_diffusion_util.py:43-96) and
    ``DDIMSampler.make_schedule`` (samplers/ddim.py:28-57), eta = 0
  * ``timestep_embedding`` (ldm_diffusion_util.py:174-194): a sinusoid table, one row per loop
    iteration.  It is computed on the host because an ulp in the frequency is amplified by t<=999
    (phase error ~6e-5 rad); a table is bit-identical to the reference's CPU value.
"""
import math
import numpy as np
import torch


def timestep_embedding_table(timesteps, dim, max_period=10000):
    t = torch.as_tensor(np.asarray(timesteps), dtype=torch.float32)
    half = dim // 2
    freqs = torch.exp(-math.log(max_period) * torch.arange(0, half, dtype=torch.float32) / half)
    args = t[:, None] * freqs[None]
    emb = torch.cat([torch.cos(args), torch.sin(args)], dim=-1)
    if dim % 2:
        emb = torch.cat([emb, torch.zeros_like(emb[:, :1])], dim=-1)
    return emb.contiguous()


def layout_betas(schedule_type, beta_start, beta_end, time_num):
    """``get_betas`` (diffusion_ddpm.py:38-84), float64.  'linear' and the three 'warm*' ramps (a linear ramp over the first 10 / 20 /
    50 % of the steps, beta_end after it).  'cosine' never reaches the loop in the reference either: its branch computes the table
    without binding it and the function fails at ``return betas`` (diffusion_ddpm.py:59-80) -- the same exception type is raised here."""
    if schedule_type == 'linear':
        return np.linspace(beta_start, beta_end, time_num).astype(np.float64)
    if schedule_type in ('warm0.1', 'warm0.2', 'warm0.5'):
        betas = beta_end * np.ones(time_num, dtype=np.float64)
        warm = int(time_num * float(schedule_type[4:]))
        betas[:warm] = np.linspace(beta_start, beta_end, warm, dtype=np.float64)
        return betas
    if schedule_type == 'cosine':
        raise UnboundLocalError("schedule_type 'cosine': the reference's get_betas returns an unbound table for it "
                                "(diffusion_ddpm.py:59-84); no model can have been trained with it")
    raise NotImplementedError(schedule_type)


class LayoutSchedule:
    """Per-iteration coefficients of the ancestral DDPM loop, iteration i <-> t = T-1-i: five numbers per step,
    ``x0 = c0 * x - c1 * out;  mean = c2 * x0 + c3 * x;  x' = mean + c4 * noise`` (ddpm_step, csrc/es_update.hip: fp contraction off).

    ``model_mean_type`` (p_mean_variance, diffusion_ddpm.py:239-257): 'eps' -> c0, c1 = sqrt(1 / ac), sqrt(1 / ac - 1);
    'x0' (the network predicts x_0 itself) -> c0, c1 = 0, -1: ``0 * x - (-1 * out)`` is ``out`` bit for bit, so the update kernel is
    the same.  ``model_var_type`` (diffusion_ddpm.py:224-235): 'fixedsmall' -> the clipped posterior log-variance; 'fixedlarge' ->
    log(cat[posterior_variance[1:2], betas[1:]]).  Either way sigma = exp(0.5 * log-variance) and no noise at t == 0."""

    def __init__(self, time_num=1000, beta_start=1e-4, beta_end=0.02, schedule_type='linear', model_mean_type='eps',
                 model_var_type='fixedsmall'):
        if model_mean_type not in ('eps', 'x0'):
            raise NotImplementedError(model_mean_type)          # (as p_mean_variance does at its first call)
        if model_var_type not in ('fixedsmall', 'fixedlarge'):
            raise NotImplementedError(model_var_type)
        self.time_num = time_num
        self.model_mean_type, self.model_var_type = model_mean_type, model_var_type
        betas64 = layout_betas(schedule_type, beta_start, beta_end, time_num)
        assert (betas64 > 0).all() and (betas64 <= 1).all()                  # diffusion_ddpm.py:134
        alphas64 = 1.0 - betas64
        ac = torch.from_numpy(np.cumprod(alphas64, axis=0)).float()        # cast to fp32 FIRST
        ac_prev = torch.from_numpy(np.append(1.0, ac[:-1])).float()
        betas = torch.from_numpy(betas64).float()
        alphas = torch.from_numpy(alphas64).float()
        post_var = betas * (1.0 - ac_prev) / (1.0 - ac)
        if model_var_type == 'fixedsmall':
            logvar = torch.log(torch.max(post_var, 1e-20 * torch.ones_like(post_var)))
        else:
            logvar = torch.log(torch.cat([post_var[1:2], betas[1:]]))
        if model_mean_type == 'eps':
            srac = torch.sqrt(1.0 / ac)
            srm1 = torch.sqrt(1.0 / ac - 1)
        else:
            srac = torch.zeros_like(ac)
            srm1 = -torch.ones_like(ac)
        c1 = betas * torch.sqrt(ac_prev) / (1.0 - ac)
        c2 = (1.0 - ac_prev) * torch.sqrt(alphas) / (1.0 - ac)
        sigma = torch.exp(0.5 * logvar)
        sigma[0] = 0.0                                                       # no noise when t == 0
        tab = torch.stack([srac, srm1, c1, c2, sigma], dim=1)               # indexed by t
        self.timesteps = np.arange(time_num - 1, -1, -1)                     # iteration order
        self.coef = tab[torch.from_numpy(self.timesteps.copy())].contiguous()   # [T, 5] by iteration
        # masked loop (keep given boxes): q_sample's two factors per iteration (GaussianDiffusion.q_sample, diffusion_ddpm.py:191-201) --
        # the reference's own tables, the square roots of the fp32 alphas_cumprod (:147-148).  A table of its own: ``coef`` stays as it is.
        # (torch.sqrt on fp32, the reference's own op: on builds that route it through a vector math library its last bit can differ
        #  between hosts, as for ``coef`` above -- whoever restates q_sample takes the factors from THIS table)
        self.sqrt_alphas_cumprod = torch.sqrt(ac).float()
        self.sqrt_one_minus_alphas_cumprod = torch.sqrt(1.0 - ac).float()
        tsi = torch.from_numpy(self.timesteps.copy())
        self.keep_tab = torch.stack([self.sqrt_alphas_cumprod[tsi], self.sqrt_one_minus_alphas_cumprod[tsi]], dim=1).contiguous()   # [T, 2] by iteration
        self.alphas_cumprod = ac                                            # fp32, by t: what a strided sampler reads (LayoutDdimSchedule)


def ddim_tables(ac, steps, eta=0.0, sqrt_1m=torch.sqrt):
    """The strided DDIM schedule over a model's fp32 ``alphas_cumprod`` [T], the ONE restatement of ``DDIMSampler.make_schedule``
    (samplers/ddim.py:28-57), ``make_ddim_timesteps('uniform')`` / ``make_ddim_sampling_parameters`` (ldm_diffusion_util.py:68-96) and the
    per-step numbers of ``p_sample_ddim`` (samplers/ddim.py:246-257), shared by the shape and the layout loop.  sigma_t as the reference
    derives it: float64 arithmetic on the fp32 alphas, ``1 - alphas`` and its reciprocal formed in fp32 first, the result cast to fp32
    when it is used; sqrt(1 - a_prev - sigma_t^2) in fp32.  Returns a dict by SCHEDULE index (ascending timesteps): ``ts`` (numpy),
    ``a``, ``a_prev``, ``sqrt_one_minus_a``, ``sigmas`` and ``cols`` = [sqrt(1-a), sqrt(a), sqrt(a_prev), sqrt(1-a_prev-sigma^2), sigma].
    The iteration count is len(ts), not necessarily ``steps``.
    ``sqrt_1m``: the square root behind ``ddim_sqrt_one_minus_alphas``.  The reference takes it with numpy (``np.sqrt(1. - ddim_alphas)``,
    samplers/ddim.py:53), which is correctly rounded; torch.sqrt on fp32 may differ from it in the last bit where the build routes it
    through a vector math library.  ShapeSchedule has always used torch.sqrt and keeps it (its tables do not change a bit); the layout
    schedule passes numpy's."""
    timesteps = int(ac.shape[0])
    c = timesteps // steps
    ts = np.asarray(list(range(0, timesteps, c))) + 1
    if ts.max() >= timesteps:
        # same failure the reference hits (IndexError in make_ddim_sampling_parameters)
        raise IndexError('ddim_steps=%d yields timestep %d >= %d' % (steps, ts.max(), timesteps))
    a = ac[ts]
    prev_list = [ac[0].item()] + ac[ts[:-1]].tolist()
    a_prev = torch.tensor(prev_list, dtype=torch.float32)
    s1m = sqrt_1m(1.0 - a)
    ap64 = np.asarray(prev_list, dtype=np.float64)
    # (the reference evaluates ``ndarray / Tensor``, i.e. Tensor.__rtruediv__ = reciprocal(1 - alphas) in fp32, times the array)
    sig64 = float(eta) * np.sqrt((1.0 - a).reciprocal().double().numpy() * (1 - ap64) * (1 - a.double().numpy() / ap64))
    sig = torch.from_numpy(sig64).to(torch.float32)
    cols = [s1m, a.sqrt(), a_prev.sqrt(), (1.0 - a_prev - sig ** 2).sqrt(), sig]
    return dict(ts=ts, a=a, a_prev=a_prev, sqrt_one_minus_a=s1m, sigmas=sig, cols=cols)


class ShapeSchedule:
    """DDIM coefficients, iteration i <-> index = S-1-i, timestep ts[index].  ``eta`` = 0 (the shipped call, echo2shape.py:484-521):
    four coefficients per step; ``eta`` != 0: sigma_t as make_ddim_sampling_parameters derives it (ddim_tables) and
    sqrt(1 - a_prev - sigma_t^2) in fp32 as p_sample_ddim forms it (samplers/ddim.py:256): five coefficients per step."""

    def __init__(self, ddim_steps=100, timesteps=1000, linear_start=0.00085, linear_end=0.012, eta=0.0):
        betas = (torch.linspace(linear_start ** 0.5, linear_end ** 0.5, timesteps,
                                dtype=torch.float64) ** 2).numpy()
        ac = torch.tensor(np.cumprod(1.0 - betas, axis=0), dtype=torch.float32)
        d = ddim_tables(ac, ddim_steps, eta)
        ts = d['ts']
        self.eta = float(eta)
        self.ddim_sigmas = d['sigmas']
        tab = torch.stack(d['cols'] if self.eta != 0.0 else d['cols'][:4], dim=1)
        order = np.arange(len(ts) - 1, -1, -1)
        self.ddim_timesteps = ts
        self.timesteps = ts[order]
        self.coef = tab[torch.from_numpy(order.copy())].contiguous()        # [S, 4 | 5] by iteration
        self.alphas_cumprod = ac
        # masked DDIM (keep given shapes, samplers/ddim.py:160-163): q_sample's two factors per iteration, from the MODEL's tables
        # (register_schedule, echo2shape.py:198-199: sqrt of the float64 cumulative product, then cast to fp32) -- not sqrt() of the
        # fp32 DDIM alphas above, which may differ in the last bit.  A table of its own: ``coef`` and its stride stay as they are.
        ac64 = np.cumprod(1.0 - betas, axis=0)
        self.sqrt_alphas_cumprod = torch.tensor(np.sqrt(ac64), dtype=torch.float32)
        self.sqrt_one_minus_alphas_cumprod = torch.tensor(np.sqrt(1.0 - ac64), dtype=torch.float32)
        tsi = torch.from_numpy(self.timesteps.copy())
        self.keep_tab = torch.stack([self.sqrt_alphas_cumprod[tsi], self.sqrt_one_minus_alphas_cumprod[tsi]], dim=1).contiguous()   # [S, 2] by iteration


LAYOUT_SAMPLERS = ('ddpm', 'ddim')


class LayoutDdimSchedule:
    """Strided DDIM on the trained layout model: the reference's model-agnostic ``DDIMSampler`` (samplers/ddim.py) driven on the layout
    denoiser, over ``layout_schedule``'s fp32 ``alphas_cumprod``.  Iteration i <-> index = S-1-i, timestep ts[index]; ``coef`` [S, 5] by
    iteration = [sqrt(1-a), sqrt(a), sqrt(a_prev), sqrt(1-a_prev-sigma^2), sigma] (ddim_tables; sigma = 0 at ``eta`` = 0, where the update
    reads no noise).  ``keep_tab`` [S, 2]: q_sample's two factors at those timesteps from the LAYOUT model's tables
    (LayoutSchedule.sqrt_alphas_cumprod / sqrt_one_minus_alphas_cumprod) -- DDIMSampler.ddim_sampling calls the model's own q_sample.
    The iteration count is len(timesteps), not necessarily ``steps``.  ``model_var_type`` plays no part in DDIM and is ignored;
    ``model_mean_type='x0'`` and ``clip_denoised=True`` have no reference arithmetic under DDIM and are refused."""

    def __init__(self, layout_schedule, steps, eta=0.0, clip_denoised=False):
        if layout_schedule.model_mean_type != 'eps':
            raise ValueError("layout DDIM: model_mean_type=%r has no reference arithmetic under DDIM (p_sample_ddim takes the network "
                             "output as eps)" % (layout_schedule.model_mean_type,))
        if clip_denoised:
            raise ValueError('layout DDIM: clip_denoised=True has no reference arithmetic under DDIM (p_sample_ddim never clips)')
        steps = int(steps)
        if steps < 1:
            raise ValueError('layout_steps must be a positive integer, got %r' % (steps,))
        self.base = layout_schedule
        self.time_num = layout_schedule.time_num
        self.eta = float(eta)
        d = ddim_tables(layout_schedule.alphas_cumprod, steps, eta, sqrt_1m=lambda v: torch.from_numpy(np.sqrt(v.numpy())))
        ts = d['ts']
        order = np.arange(len(ts) - 1, -1, -1)
        self.ddim_timesteps = ts
        self.ddim_alphas, self.ddim_alphas_prev = d['a'], d['a_prev']
        self.ddim_sqrt_one_minus_alphas, self.ddim_sigmas = d['sqrt_one_minus_a'], d['sigmas']
        self.timesteps = ts[order]
        self.coef = torch.stack(d['cols'], dim=1)[torch.from_numpy(order.copy())].contiguous()     # [S, 5] by iteration
        tsi = torch.from_numpy(self.timesteps.copy())
        self.keep_tab = torch.stack([layout_schedule.sqrt_alphas_cumprod[tsi], layout_schedule.sqrt_one_minus_alphas_cumprod[tsi]],
                                    dim=1).contiguous()                                            # [S, 2] by iteration


SHAPE_SAMPLERS = ('ddim', 'plms')


def plms_evaluations(n_timesteps, n_steps=None):
    """The denoiser evaluations of a PLMS run (PLMSSampler.plms_sampling / p_sample_plms, samplers/plms.py:149-247) over a schedule of
    ``n_timesteps`` timesteps, in order, as (table row, kind): the row of the per-iteration tables (ShapeSchedule.timesteps, the
    time-embedding table) the evaluation reads, and what consumes its eps --
        'first'   iteration 0, first evaluation (row 0): improved Euler's predictor (es_plms_first_a); its eps enters the history;
        'second'  iteration 0, second evaluation at the NEXT timestep (row 1, the reference's t_next): the corrector (es_plms_first_b);
        'steady'  iteration i >= 1 (row i): Adams-Bashforth on the eps of the last min(i, 3) iterations (es_plms_update).
    ``n_steps`` iterations (None: all) make n_steps + 1 evaluations."""
    n = int(n_timesteps) if n_steps is None else int(n_steps)
    if n_timesteps < 2:
        raise ValueError('PLMS needs at least 2 timesteps')
    if n < 0 or n > n_timesteps:
        raise ValueError('n_steps must be in [0, %d]' % n_timesteps)
    if n == 0:
        return []
    return [(0, 'first'), (1, 'second')] + [(i, 'steady') for i in range(1, n)]
