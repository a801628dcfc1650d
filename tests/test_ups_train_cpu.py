"""The algebra of the upsample convolutions' training path (kern.GemmFn's transposed form), in float64 on the CPU against
`F.conv2d(F.interpolate(x, 2), w, padding=1)` and its autograd gradients: the tap sets, the parity <-> W4 index map of
the forward operand and the fold map of the weight gradient -- the host restatements (kern.ups_composite / ups_fold) of
what sdmi_pack_dgrad's composite modes and sdmi_ups_fold_dw do on the device.  No kernel is launched here."""
import pytest
import torch
import torch.nn.functional as F

from slotdiffusion_amd import bwd, kern

F64 = torch.float64
SHAPES = [(2, 3, 4, 5, 6), (1, 1, 1, 2, 3), (2, 4, 3, 1, 1)]      # B, H, W, Cin, Cout


def _case(shape, seed=0):
    B, H, W, ci, co = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, ci, H, W, dtype=F64, generator=g, requires_grad=True)
    w = torch.randn(co, ci, 3, 3, dtype=F64, generator=g, requires_grad=True)
    dy = torch.randn(B, co, 2 * H, 2 * W, dtype=F64, generator=g)
    y = F.conv2d(F.interpolate(x, scale_factor=2, mode='nearest'), w, padding=1)
    dx, dw = torch.autograd.grad(y, [x, w], dy)
    return x.detach(), w.detach(), dy, y.detach(), dx, dw


def test_tap_sets_partition_the_filter():
    """Every source tap lands in exactly two composite taps per dimension's pair of parities: the sets of one parity
    ({3, 1} or {2, 0}) partition {0, 1, 2}."""
    for par in (0, 1):
        taps = sorted(k for r in (0, 1) for k in kern.UPS_TAPS[3 - 2 * r - par])
        assert taps == [0, 1, 2]
    assert kern.UPS_TAPS == ((2,), (1, 2), (0, 1), (0,))


@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_forward_is_the_transposed_convolution_of_the_composite_filter(shape):
    x, w, dy, y, dx, dw = _case(shape)
    w4 = kern.ups_composite(w)
    yt = F.conv_transpose2d(x, w4.permute(1, 0, 2, 3), stride=2, padding=1)
    assert float((yt - y).abs().max()) <= 1e-13 * max(1.0, float(y.abs().max()))


@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_parity_filters_are_w4_taps(shape):
    """Tap (r, c) of output parity (py, px) in ups_parity_split -- the `parity4` operand -- is W4[3 - 2r - py][3 - 2c - px],
    bit for bit (same sums in the same order)."""
    _, w, *_ = _case(shape)
    co, ci = w.shape[:2]
    w4 = kern.ups_composite(w.float())
    parts = kern.ups_parity_split(w.float())
    for py in (0, 1):
        for px in (0, 1):
            p = parts[py, px].view(co, 2, 2, ci)
            for r in (0, 1):
                for c in (0, 1):
                    assert torch.equal(p[:, r, c, :], w4[:, :, 3 - 2 * r - py, 3 - 2 * c - px]), (py, px, r, c)


@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_data_gradient_is_the_strided_convolution(shape):
    x, w, dy, y, dx, dw = _case(shape)
    w4 = kern.ups_composite(w)
    dxs = F.conv2d(dy, w4.permute(1, 0, 2, 3), stride=2, padding=1)
    assert dxs.shape == dx.shape
    assert float((dxs - dx).abs().max()) <= 1e-13 * max(1.0, float(dx.abs().max()))


@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_weight_gradient_folds_back(shape):
    """dW4 = the weight gradient of that strided convolution with the roles swapped (image dY, output gradient x), folded
    by ups_fold, is autograd's dw."""
    x, w, dy, y, dx, dw = _case(shape)
    w4 = kern.ups_composite(w).permute(1, 0, 2, 3).contiguous().requires_grad_(True)       # [Cin][Cout][4][4]
    (dw4,) = torch.autograd.grad(F.conv2d(dy, w4, stride=2, padding=1), [w4], x)
    got = kern.ups_fold(dw4.permute(1, 0, 2, 3))
    assert float((got - dw).abs().max()) <= 1e-13 * max(1.0, float(dw.abs().max()))


def test_layer_problem_of_the_transposed_form():
    """bwd.LayerProblem.upsampled: the 4x4 stride-2 pad-1 convolution dY -> dx with the roles swapped."""
    x = torch.empty(3, 4, 8, 64, dtype=torch.bfloat16)
    P = bwd.LayerProblem.upsampled(x, 192)
    assert (P.B, P.H, P.W, P.Ho, P.Wo, P.Cin, P.N, P.K, P.M) == (3, 8, 16, 4, 8, 192, 64, 16 * 192, 3 * 4 * 8)
    assert (P.kh, P.kw, P.stride, P.pad, P.ups, P.lda, P.ldy) == (4, 4, 2, (1, 1, 1, 1), False, 192, 64)
    assert bwd.standalone_splits(P) == 1
