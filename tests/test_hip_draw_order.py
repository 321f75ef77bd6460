"""The order of the device RNG draws of the sampling loops is a contract ("emit / compose / stage"): ranks seeded alike
must stay in step, and a caller who seeds the generator and passes no noise gets what the same draws, made by hand in that order
and passed in, give -- bit for bit.
  layout:  the keep table [T, O * 8], then ``noise`` [T + 1, O, 8]
  shape:   the keep table [S, O * latent], then ``noise1`` [1, C, D, H, W], then ``step_noise`` [S, O * latent] (eta != 0 only)
  fused:   layout keep, layout noise, shape keep, shape ``noise1`` (then, eta != 0 only and not tested here, the step-noise table)
Tiny models: the layout denoiser of test_hip_keep_boxes.py's ``tiny`` (O = 8, T = 100) and test_hip_keep.py's ``_shape`` (O = 4, 16^3
latents, S = 4)."""
import pytest
import torch

from conftest import load_golden
from test_hip_keep import _shape, _keep_inputs, _rnd

pytestmark = pytest.mark.gpu
Z = (3, 16, 16, 16)
PER = 3 * 16 ** 3


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda')


@pytest.fixture(scope='module')
def lay(dev):
    from test_hip_rows import _layout
    return _layout(dev, 128, 128, 'unet1d_tiny.', 100)


@pytest.fixture(scope='module')
def shp(dev):
    return _shape(dev)


def test_layout_masked_draws_keep_table_then_noise(dev, lay):
    g, gp = load_golden('layout_keep_tiny'), load_golden('layout_loop_tiny')
    oe, triples, x0 = gp['obj_embed'], gp['triples'], g['x0']
    mask = torch.zeros(8)
    mask[g['keep'].long()] = 1.0
    T = lay.T
    torch.manual_seed(11)
    drawn = lay.sample(oe, triples, x0=x0, mask=mask)
    torch.manual_seed(11)
    kn = torch.randn(T, 8 * 8, device=dev)
    noise = torch.randn(T + 1, 8, 8, device=dev)
    given = lay.sample(oe, triples, noise, x0=x0, mask=mask, keep_noise=kn.reshape(T, 8, 8))
    assert torch.equal(drawn, given)


def test_shape_draws_keep_table_noise1_then_step_noise(dev, shp):
    g = load_golden('ddim_keep_tiny')
    x0, mask, _ = _keep_inputs(g)
    uc, triples, S = g['uc_s'], g['triples'], shp.S
    torch.manual_seed(12)
    drawn = shp.sample(uc, triples, x0=x0, mask=mask)
    torch.manual_seed(12)
    kn = torch.randn(S, 4 * PER, device=dev)
    n1 = torch.randn((1,) + Z, device=dev)
    given = shp.sample(uc, triples, n1, x0=x0, mask=mask, keep_noise=kn.reshape((S, 4) + Z))
    assert torch.equal(drawn, given)
    # eta != 0, unmasked: noise1, then the per-step table
    eta = _shape(dev, ddim_eta=0.5, weights=shp.w)
    torch.manual_seed(13)
    drawn = eta.sample(uc, triples)
    torch.manual_seed(13)
    n1 = torch.randn((1,) + Z, device=dev)
    sn = torch.randn(S, 4 * PER, device=dev)
    given = eta.sample(uc, triples, n1, step_noise=sn.reshape((S, 4) + Z))
    assert torch.equal(drawn, given)


def test_fused_call_draws_layout_keep_layout_noise_shape_keep_noise1(dev, lay, shp):
    from echoscene_amd.samplers import sample_layout_and_shape
    g, gp = load_golden('ddim_keep_tiny'), load_golden('layout_loop_tiny')
    x0, mask, _ = _keep_inputs(g)
    uc, triples, S, T = g['uc_s'], g['triples'], shp.S, lay.T
    oe = gp['obj_embed'][:4]
    bx0, bmask = _rnd((4, 8), 21, 0.5), torch.tensor([1.0, 0.0, 0.0, 1.0])
    kw = dict(x0=x0, mask=mask, box_x0=bx0, box_mask=bmask)
    torch.manual_seed(14)
    xd, zd = sample_layout_and_shape(lay, shp, oe, triples, uc, **kw)
    torch.manual_seed(14)
    bkn = torch.randn(T, 4 * 8, device=dev)
    ln = torch.randn(T + 1, 4, 8, device=dev)
    kn = torch.randn(S, 4 * PER, device=dev)
    n1 = torch.randn((1,) + Z, device=dev)
    xg, zg = sample_layout_and_shape(lay, shp, oe, triples, uc, layout_noise=ln, shape_noise=n1, keep_noise=kn.reshape((S, 4) + Z),
                                     box_keep_noise=bkn.reshape(T, 4, 8), **kw)
    assert torch.equal(xd, xg) and torch.equal(zd, zg)
