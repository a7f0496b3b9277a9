"""GPU: houv_kabsch against the float64 restatement of SVDHead's contract (tests/kabsch_host.py) on both load paths (16-byte
vector loads; scalar loads when N is no multiple of 4 or a base is not 16-byte aligned), idle lanes, early-returning waves,
weights, the reflection branch and clouds far from the origin (what the kernel's shift about the first point is for).

Bound per case, R and t separately: 4 x the error of the SAME contract evaluated two-pass in float32 on the same inputs, plus
8 x 2^-24 x max |value| (kabsch_host.reference_and_bounds).  The yardstick comes from the reference, never from the kernel;
DESIGN.md section 9.3 tabulates yardstick, kernel error and bound per case."""
import ctypes

import numpy as np
import pytest
import torch

import kabsch_host as host

pytestmark = pytest.mark.gpu

# (N, B).  N in {1, 3, 37, 63, 64, 65, 257, 2050}: no multiple of 4 -> scalar path, below 64 with idle lanes; {40, 256, 2048}:
# vector path.  B = 5: the second workgroup has three waves that return early; B = 1 and 4 at one size of either path.
SIZES = [(3, 5), (37, 1), (37, 4), (37, 5), (63, 5), (64, 5), (65, 5), (257, 5), (2050, 5),
         (40, 1), (40, 4), (40, 5), (256, 5), (2048, 5)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _run(dev, src, corr, w):
    from houv_amd import ops
    R, t = ops.kabsch(torch.tensor(src).to(dev), torch.tensor(corr).to(dev), None if w is None else torch.tensor(w).to(dev))
    return R.cpu().numpy(), t.cpu().numpy()


def _check(tag, R, t, B, N, weighted, offset, reflect):
    R64, t64, yard, bound = host.reference_and_bounds(B, N, weighted, offset, reflect)
    eR, et = host.errors(R, t, R64, t64)
    print(f"KABSCH {tag} N={N} B={B} w={int(weighted)} off={int(offset)} refl={int(reflect)} "
          f"yard_R={yard[0]:.2e} err_R={eR:.2e} bound_R={bound[0]:.2e} yard_t={yard[1]:.2e} err_t={et:.2e} bound_t={bound[1]:.2e}")
    assert eR <= bound[0], (eR, bound[0])
    assert et <= bound[1], (et, bound[1])
    det = np.linalg.det(R.astype(np.float64))
    assert (np.abs(det - 1) < 1e-5).all(), det                     # a rotation, also on the reflection branch


@pytest.mark.parametrize("reflect", [False, True], ids=["plain", "mirrored"])
@pytest.mark.parametrize("offset", [False, True], ids=["origin", "far"])
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("N,B", SIZES)
def test_kabsch_within_four_float32_yardsticks(dev, N, B, weighted, offset, reflect):
    src, corr, w = host.make_case(B, N, weighted, offset, reflect)
    R, t = _run(dev, src, corr, w)
    _check("case", R, t, B, N, weighted, offset, reflect)


@pytest.mark.parametrize("offset", [False, True], ids=["origin", "far"])
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
def test_kabsch_single_point(dev, weighted, offset):
    """N = 1: every moment about the first point is 0, so H = 0 exactly; R is whatever kabsch_rotation makes of the zero matrix
    (the host build of the same header says what), a proper rotation, and t = corr - R src (times the weight when weighted).
    Floor: 8 roundings of the largest operand -- t itself can be small where src and corr are 100 away."""
    from tests import hostmath
    B = 5
    src, corr, w = host.make_case(B, 1, weighted, offset, False)
    R, t = _run(dev, src, corr, w)
    fp = ctypes.POINTER(ctypes.c_float)
    R0 = np.zeros(9, np.float32)
    hostmath.load().hm_kabsch_rotation_f32(np.zeros(9, np.float32).ctypes.data_as(fp), 1, R0.ctypes.data_as(fp))
    np.testing.assert_array_equal(R, np.broadcast_to(R0.reshape(3, 3), (B, 3, 3)))
    assert abs(np.linalg.det(R0.reshape(3, 3).astype(np.float64)) - 1) < 1e-6
    s, c = src[:, :, 0].astype(np.float64), corr[:, :, 0].astype(np.float64)
    if weighted:
        s, c = s * w[:, 0].astype(np.float64), c * w[:, 0].astype(np.float64)
    want = c - np.einsum("bij,bj->bi", R.astype(np.float64), s)
    floor = 8 * host.EPS32 * max(np.abs(s).max(), np.abs(c).max(), np.abs(want).max())
    assert np.abs(t - want).max() <= floor, (np.abs(t - want).max(), floor)


@pytest.mark.parametrize("offset", [False, True], ids=["origin", "far"])
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
def test_kabsch_unaligned_base_takes_the_scalar_path(dev, weighted, offset):
    """[B,3,40] views that start one float into a larger buffer: contiguous, N a multiple of 4, but not 16-byte aligned, so the
    16-byte loads must not be used.  Same data, same bound as the aligned copy."""
    from houv_amd import ops
    B, N = 5, 40
    src, corr, w = host.make_case(B, N, weighted, offset, False)

    def shifted(a):
        buf = torch.zeros(a.size + 8, dtype=torch.float32, device=dev)
        v = buf[1:1 + a.size].view(a.shape)
        v.copy_(torch.tensor(a))
        assert v.is_contiguous() and v.data_ptr() % 16 == 4
        return v

    R, t = ops.kabsch(shifted(src), shifted(corr), None if w is None else shifted(w))
    _check("unaligned", R.cpu().numpy(), t.cpu().numpy(), B, N, weighted, offset, False)
    if weighted:                                                    # aligned clouds, unaligned weights alone
        R, t = ops.kabsch(torch.tensor(src).to(dev), torch.tensor(corr).to(dev), shifted(w))
        _check("unaligned-w", R.cpu().numpy(), t.cpu().numpy(), B, N, weighted, offset, False)
