"""The identity behind the folded up-sampling conv (csrc/small.hip: upconv_fold_kernel, csrc/upconv.hip: conv3x3_upfold_kernel),
pinned in float64 without a GPU.

    y = conv3x3(up2(x), w, pad 1),   up2 = F.interpolate(scale_factor=2, mode="bilinear", align_corners=False)

Output pixel (2i + a, 2j + b) is a 3x3 conv of the replicate-padded LOW-resolution input with the weights of phase (a, b),
    Wf[a][b][r][s] = sum_{u,v} R[a][r][u] R[b][s][v] w[u][v],
except on the outermost ring of the output, where the conv's zero padding must win over the bilinear clamp: kernel row ue = 0
is dropped for (a = 0, i = 0), row 2 for (a = 1, i = H - 1), columns alike.  As corrections to the interior form: three taps on
the centre patch row for the pixels of that image row, three on the centre column, one at the corner (subtracted twice).

fold_blob_f64 builds the 64 weight sets in the order the kernels use (csrc/kernels.h); folded_conv_f64 applies them the way the
kernel does.  The GPU tests (test_gpu_upconv_fold.py) reuse both."""
import pytest
import torch
import torch.nn.functional as F

# R[a][r][u]: weight of low-resolution row i + r - 1 in up-sampled row 2i + a + u - 1
R = torch.tensor([[[.75, .25, 0.], [.25, .75, .75], [0., 0., .25]],
                  [[.25, 0., 0.], [.75, .75, .25], [0., .25, .75]]], dtype=torch.float64)


def fold_blob_f64(w):
    """w [O][I][3][3] -> [64][O][I] float64: sets p * 9 + r * 3 + s (interior), 36 + p * 3 + s (row edge, negated),
    48 + p * 3 + r (column edge, negated), 60 + p (corner); p = 2 a + b."""
    w = w.double()
    sets = [None] * 64
    for a in range(2):
        for b in range(2):
            p, ue, ve = 2 * a + b, 2 * a, 2 * b
            for r in range(3):
                for s in range(3):
                    sets[p * 9 + r * 3 + s] = torch.einsum("u,v,oiuv->oi", R[a][r], R[b][s], w)
            for s in range(3):
                sets[36 + p * 3 + s] = -torch.einsum("v,oiv->oi", R[b][s], w[:, :, ue, :])
            for r in range(3):
                sets[48 + p * 3 + r] = -torch.einsum("u,oiu->oi", R[a][r], w[:, :, :, ve])
            sets[60 + p] = w[:, :, ue, ve].clone()
    return torch.stack(sets)


def folded_conv_f64(x, blob, bias):
    """x [B][I][H][W], blob [64][O][I] (fold_blob_f64 layout, any dtype) -> [B][O][2H][2W] float64."""
    x, blob = x.double(), blob.double()
    B, _, H, W = x.shape
    O = blob.shape[1]
    xr = F.pad(x, (1, 1, 1, 1), mode="replicate")
    y = torch.zeros(B, O, 2 * H, 2 * W, dtype=torch.float64)

    def mm(wset, t):  # [O][I] x [B][I][...] -> [B][O][...]
        return torch.einsum("oi,bi...->bo...", wset, t)

    for a in range(2):
        for b in range(2):
            p = 2 * a + b
            ie, je = (H - 1) * a, (W - 1) * b
            yp = torch.zeros(B, O, H, W, dtype=torch.float64)
            for r in range(3):
                for s in range(3):
                    yp += mm(blob[p * 9 + r * 3 + s], xr[:, :, r:r + H, s:s + W])
            for s in range(3):  # edge row: three taps on the centre patch row
                yp[:, :, ie, :] += mm(blob[36 + p * 3 + s], xr[:, :, ie + 1, s:s + W])
            for r in range(3):  # edge column: three taps on the centre patch column
                yp[:, :, :, je] += mm(blob[48 + p * 3 + r], xr[:, :, r:r + H, je + 1])
            yp[:, :, ie, je] += mm(blob[60 + p], x[:, :, ie, je])
            y[:, :, a::2, b::2] = yp
    return y + bias.double().view(1, -1, 1, 1)


def upconv_ref_f64(x, w, bias):
    up = F.interpolate(x.double(), scale_factor=2, mode="bilinear", align_corners=False)
    return F.conv2d(up, w.double(), bias.double(), padding=1)


@pytest.mark.parametrize("hw", [(1, 1), (2, 3), (1, 5), (8, 16), (7, 4)])
def test_folded_weights_and_border_corrections_equal_interpolate_then_conv(hw):
    """Interior sets plus the masked corrections against F.interpolate + F.conv2d in float64, to 1e-12 relative."""
    g = torch.Generator().manual_seed(hw[0] * 100 + hw[1])
    x = torch.randn(2, 5, *hw, generator=g, dtype=torch.float64)
    w = torch.randn(4, 5, 3, 3, generator=g, dtype=torch.float64)
    b = torch.randn(4, generator=g, dtype=torch.float64)
    ref = upconv_ref_f64(x, w, b)
    got = folded_conv_f64(x, fold_blob_f64(w), b)
    assert got.shape == ref.shape
    assert (got - ref).abs().max().item() < 1e-12 * ref.abs().max().item()


def test_fold_coefficients_are_sixteenths_of_at_most_49():
    """Every fold coefficient is a multiple of 1/16 and at most 49/16 in magnitude (w = 1 shows the largest: the sum over a
    set), so the fold adds no rounding of its own before the one to the compute dtype."""
    blob = fold_blob_f64(torch.ones(1, 1, 3, 3))
    assert torch.equal(blob * 16, (blob * 16).round())
    assert blob.abs().max().item() == 49 / 16
