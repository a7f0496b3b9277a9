"""CPU: the term-mask rule of the pruned solve (houv::term_masks, houv_amd/csrc/houv_math.h), run as a stand-alone host program.

The rule drops a Chamfer term (direction Y of metric m) for the coming iteration when, at an anchor iteration that computed all
eight terms, cd_X + 2 d + margin < cd_Y, d bounding how far any moved point has travelled since.  Soundness is checked against
float64 numpy: random clouds of 64..128 points, random poses, random small motions sized around the gap between the two
directions (so the draws straddle the threshold); whenever the rule drops a term, that term truly loses the min at the new pose.
The rule sees what the kernel would give it: fp32 poses, the fp32 roundings of the anchor's terms, an fp32 radius."""
import numpy as np
import pytest

from tests import termmasks

ANCHORS, MOTIONS = 1280, 8          # 10,240 draws
BATCH = 64


def _rot(axis, angle):
    """Rodrigues, float64 [n,3,3]."""
    axis = axis / np.linalg.norm(axis, axis=1, keepdims=True)
    x, y, z = axis[:, 0], axis[:, 1], axis[:, 2]
    zero = np.zeros_like(x)
    A = np.stack([zero, -z, y, z, zero, -x, -y, x, zero], 1).reshape(-1, 3, 3)
    s, c = np.sin(angle)[:, None, None], np.cos(angle)[:, None, None]
    return np.eye(3)[None] + s * A + (1.0 - c) * (A @ A)


def _terms(src, tgt, R, T):
    """The eight terms of Predict_loss in float64: cd[b, metric, dir], dir 0 over the target points, 1 over the moved points;
    metric 0 = mean of the k = N/2 smallest distances, metrics 1..3 = mean over all points with axis m-1 dropped."""
    moved = src @ np.swapaxes(R, 1, 2) + T[:, None, :]
    d2 = (moved[:, :, None, :] - tgt[:, None, :, :]) ** 2                    # [b, n(moved), m(target), 3]
    full = d2.sum(-1)
    cd = np.empty((src.shape[0], 4, 2))
    k = src.shape[1] // 2
    for m, sq in enumerate((full, full - d2[..., 0], full - d2[..., 1], full - d2[..., 2])):
        sq = np.maximum(sq, 0.0)
        over_moved, over_target = np.sqrt(sq.min(2)), np.sqrt(sq.min(1))
        if m == 0:
            over_moved, over_target = np.sort(over_moved, 1)[:, :k], np.sort(over_target, 1)[:, :k]
        cd[:, m, 0], cd[:, m, 1] = over_target.mean(1), over_moved.mean(1)
    return cd


def _records(cd_anchor, Ra, Ta, R, T, radius):
    n = cd_anchor.shape[0]
    return np.concatenate([cd_anchor.reshape(n, 8), Ra.reshape(n, 9), Ta, R.reshape(n, 9), T, radius.reshape(n, 1)],
                          axis=1).astype(np.float32)


def test_a_dropped_term_truly_loses_over_ten_thousand_draws():
    rng = np.random.default_rng(2024)
    dropped = kept_with_gap = draws = 0
    for b0 in range(0, ANCHORS, BATCH):
        n_pts = int(rng.integers(64, 129))
        # a target that is a cropped, noisy, rigidly displaced copy plus clutter: the two directions differ, metric by metric
        src = rng.standard_normal((BATCH, n_pts, 3)).astype(np.float32).astype(np.float64) * 0.4
        keep = int(n_pts * rng.uniform(0.5, 1.0))
        tgt = src.copy()
        tgt[:, keep:] = rng.standard_normal((BATCH, n_pts - keep, 3)) * rng.uniform(0.2, 1.0)
        tgt = (tgt + rng.standard_normal(tgt.shape) * 0.01).astype(np.float32).astype(np.float64)
        Ra = _rot(rng.standard_normal((BATCH, 3)), rng.uniform(0, np.pi, BATCH)).astype(np.float32).astype(np.float64)
        Ta = rng.uniform(-0.25, 0.25, (BATCH, 3)).astype(np.float32).astype(np.float64)
        radius = np.sqrt((src ** 2).sum(-1).max(1))
        cd_a = _terms(src, tgt, Ra, Ta)
        gap = np.abs(cd_a[:, :, 0] - cd_a[:, :, 1])                              # [b, 4]
        for _ in range(MOTIONS):
            # motion sized to a random metric's gap: 2 d between 0 and 2.5 gaps
            g = gap[np.arange(BATCH), rng.integers(0, 4, BATCH)]
            d = rng.uniform(0.0, 1.25, BATCH) * g * 0.5
            share = rng.uniform(0.0, 1.0, BATCH)                                 # of d spent on the rotation
            dR = _rot(rng.standard_normal((BATCH, 3)), share * d / (np.sqrt(2.0) * radius))
            dT = rng.standard_normal((BATCH, 3))
            dT *= ((1.0 - share) * d / np.linalg.norm(dT, axis=1))[:, None]
            R = (dR @ Ra).astype(np.float32).astype(np.float64)
            T = (Ta + dT).astype(np.float32).astype(np.float64)
            need = termmasks.run(_records(cd_a, Ra, Ta, R, T, radius))
            cd_t = _terms(src, tgt, R, T)
            for m in range(4):
                need0, need1 = (need >> m) & 1, (need >> (4 + m)) & 1
                assert ((need0 | need1) == 1).all()                              # never both
                lose0, lose1 = need0 == 0, need1 == 0
                assert (cd_t[lose0, m, 0] > cd_t[lose0, m, 1]).all(), "dropped dir 0 although it wins or ties"
                assert (cd_t[lose1, m, 1] > cd_t[lose1, m, 0]).all(), "dropped dir 1 although it wins or ties"
                dropped += int(lose0.sum() + lose1.sum())
                kept_with_gap += int(((need0 & need1) == 1).sum())
            draws += BATCH
    assert draws >= 10000
    # the rule is not vacuous and the draws straddle its threshold: a solid share of the terms dropped, a solid share kept
    assert dropped > draws * 4 // 10 and kept_with_gap > draws * 4 // 10, (dropped, kept_with_gap, draws)


def _one(cd, Ra=None, Ta=None, R=None, T=None, radius=1.0, nmet=4):
    eye = np.eye(3, dtype=np.float32)
    Ra = eye if Ra is None else Ra
    R = Ra if R is None else R
    Ta = np.zeros(3, np.float32) if Ta is None else Ta
    T = Ta if T is None else T
    rec = _records(np.asarray(cd, np.float64).reshape(1, 4, 2), np.asarray(Ra)[None], np.asarray(Ta)[None],
                   np.asarray(R)[None], np.asarray(T)[None], np.asarray([radius]))
    return int(termmasks.run(rec, nmet)[0])


def test_a_clear_gap_drops_the_loser_and_only_the_loser():
    cd = [[0.1, 0.5], [0.5, 0.1], [0.2, 0.2002], [0.3, 0.3]]
    assert _one(cd) == 0xFF & ~(1 << 4) & ~(1 << 1)          # metric 0: dir 1 loses; metric 1: dir 0 loses; 2, 3: too close
    assert _one(cd, nmet=1) == 0x01                          # single-metric twin: one bit per direction
    # the same gap, but the cloud has moved by more than half of it
    assert _one(cd, T=np.array([0.25, 0.0, 0.0], np.float32)) == 0xFF


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf")])
def test_nan_and_inf_keep_both_terms(bad):
    base = [[0.1, 0.5]] * 4
    for d in (0, 1):
        cd = [row[:] for row in base]
        cd[2][d] = bad
        need = _one(cd)
        assert (need >> 2) & 1 and (need >> 6) & 1, hex(need)
        assert need & ~0x44 == 0xFF & ~0x44 & ~0xB0              # the other metrics still drop their dir 1
    Rbad = np.eye(3, dtype=np.float32)
    Rbad[1, 1] = bad
    Tbad = np.array([0.0, bad, 0.0], np.float32)
    assert _one(base, R=Rbad) == 0xFF and _one(base, Ra=Rbad, R=np.eye(3, dtype=np.float32)) == 0xFF
    assert _one(base, T=Tbad) == 0xFF and _one(base, Ta=Tbad, T=np.zeros(3, np.float32)) == 0xFF
    assert _one(base, radius=bad) == 0xFF                    # 0 * inf included: the pose has not moved


def test_ties_keep_both_terms():
    assert _one([[0.25, 0.25]] * 4) == 0xFF
    assert _one([[0.0, 0.0]] * 4) == 0xFF
    one_ulp = np.nextafter(np.float32(0.25), np.float32(1))
    assert _one([[0.25, one_ulp], [one_ulp, 0.25], [0.25, 0.25], [0.25, 0.25]]) == 0xFF
