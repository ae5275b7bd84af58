"""The BatchNorm and dropout row kernels (``dv_bn_fwd`` / ``dv_bn_bwd`` / ``dv_mask_scale``) launched directly, against the
float64 references and componentwise bounds of tests/mmd_bn_ref.py (held themselves by tests/test_mmd_bn_ref_cpu.py).

Shapes cross the kernels' strides: 64 columns per workgroup (N = 63, 64, 65, 130: ``blockIdx.x > 0``), four row groups
(M = 2, 3, 5, 67).  Every operand is a row-strided view (ld = width + 3 or + 5) in a buffer whose pads and guard rows hold
NaN, every output sits in a buffer pre-filled with a sentinel that must survive bit for bit, and every launch runs twice
and must store the same bits."""
import pytest
import torch
import torch.nn.functional as F

from tests import mmd_bn_ref as R, ref64

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def K(dev):
    import drvae_amd.kernels as K
    from drvae_amd import _lib
    _lib.load()
    return K


@pytest.mark.parametrize('N', R.BN_N)
@pytest.mark.parametrize('M', R.BN_M)
def test_bn_fwd(K, dev, M, N):
    """training and eval, the affine pair and the running statistics given and None, momentum 0.1 and 1.0, eps 1e-5 and
    0 (the latter without the constant column): mean, rstd, y and both running statistics"""
    res = {}
    for mode in R.BN_FWD_MODES:
        for k, v in R.run_bn_fwd(K, dev, M, N, mode).items():
            res[k] = max(res.get(k, 0.0), v)
    R.report(res)


def test_bn_fwd_one_row_eval(K, dev):
    """M = 1 is ``blocks.BatchNorm1d``'s own error when training; in eval mode the launch takes it"""
    R.report(R.run_bn_fwd(K, dev, 1, 65, R.BN_FWD_MODES[4]))


@pytest.mark.parametrize('N', R.BN_N)
@pytest.mark.parametrize('M', R.BN_M)
def test_bn_bwd(K, dev, M, N):
    """training and eval, dx / dw / db each None in turn, the weight given and None, dy with a column of zeros"""
    res = {}
    for mode in R.BN_BWD_MODES:
        for k, v in R.run_bn_bwd(K, dev, M, N, mode).items():
            res[k] = max(res.get(k, 0.0), v)
    R.report(res)


@pytest.mark.parametrize('scale', R.MASK_SCALES)
@pytest.mark.parametrize('M,N', R.MASK_SHAPES)
def test_mask_scale(K, dev, M, N, scale):
    """exact: the fp32 product x * mask * scale in that order, out of place and with y being x (what chain.py relies on)"""
    R.run_mask_scale(K, dev, M, N, scale)


def test_mask_scale_empty(K, dev):
    """M = 0 and N = 0 return without a launch: nothing is written"""
    for M, N in ((0, 5), (5, 0)):
        fr = R.Frame(dev)
        y = fr.out((5, 5))
        x, mask = torch.ones(M, N, device=dev), torch.ones(M, N, device=dev)
        K.mask_scale(y[:M, :N], x, mask, 2.0)
        fr.verify(untouched=True)


def test_batch_norm_and_dropout_modules(dev, K, monkeypatch):
    """``blocks.BatchNorm1d`` and ``blocks.Dropout`` at (67, 130), forward and backward, against float64
    ``F.batch_norm`` and its autograd under the same bounds (the saved statistics enter the backward's bound with the
    forward's bounds on them); dropout is the exact fp32 product both ways"""
    import drvae_amd.blocks as blk
    M, N = 67, 130
    x, p = R.bn_input(M, N), R.bn_params(N)
    dy = torch.randn(M, N, generator=torch.Generator().manual_seed(3))
    bn = blk.BatchNorm1d(N).to(dev)
    with torch.no_grad():
        bn.weight.copy_(p['w'])
        bn.bias.copy_(p['b'])
        bn.running_mean.copy_(p['rm'])
        bn.running_var.copy_(p['rv'])
    res = {}
    for training in (True, False):
        bn.train(training)
        rm0, rv0 = bn.running_mean.cpu().clone(), bn.running_var.cpu().clone()
        xd = x.clone().to(dev).requires_grad_(True)
        y = bn(xd)
        (y * dy.to(dev)).sum().backward()
        x64 = x.double().requires_grad_(True)
        w64, b64 = p['w'].double().requires_grad_(True), p['b'].double().requires_grad_(True)
        rm64, rv64 = rm0.double(), rv0.double()
        y64 = F.batch_norm(x64, rm64, rv64, w64, b64, training, ref64.f32(0.1), ref64.f32(1e-5))
        (y64 * dy.double()).sum().backward()
        r = R.bn_fwd(x, p['w'], p['b'], rm0, rv0, 1e-5, 0.1, training)
        tag = 'BatchNorm1d %s ' % ('train' if training else 'eval')
        res[tag + 'y'] = ref64.check(tag + 'y', y, y64.detach(), r['y_b'])
        if training:
            res[tag + 'running_mean'] = ref64.check(tag + 'running_mean', bn.running_mean, rm64, r['running_mean_b'])
            res[tag + 'running_var'] = ref64.check(tag + 'running_var', bn.running_var, rv64, r['running_var_b'])
        b = R.bn_bwd(dy, x, r['mean'], r['rstd'], p['w'], training, e_mean=r['mean_b'], e_rstd=r['rstd_b'])
        res[tag + 'dx'] = ref64.check(tag + 'dx', xd.grad, x64.grad, b['dx_b'])
        res[tag + 'dw'] = ref64.check(tag + 'dw', bn.weight.grad, w64.grad, b['dw_b'])
        res[tag + 'db'] = ref64.check(tag + 'db', bn.bias.grad, b64.grad, b['db_b'])
        bn.weight.grad = bn.bias.grad = None
    assert int(bn.num_batches_tracked) == 1
    R.report(res)
    xm, mask = R.mask_case(M, N)
    monkeypatch.setattr(blk, '_keep_mask_like', lambda t, keep: mask.to(dev).clone())
    drop = blk.Dropout(p=0.1).to(dev).train()
    xd = xm.clone().to(dev).requires_grad_(True)
    yd = drop(xd)
    yd.backward(dy.to(dev))
    assert R.same_bits(yd.detach().cpu(), R.mask_scale(xm, mask, 1.0 / (1.0 - 0.1)))
    assert R.same_bits(xd.grad.cpu(), R.mask_scale(dy, mask, 1.0 / (1.0 - 0.1)))
    assert drop.eval()(xd) is xd
