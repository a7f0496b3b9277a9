"""CPU: the per-term-record rule of the pruned solve (houv::term_anchor_masks, houv_amd/csrc/houv_math.h), run as a stand-alone
host program beside houv::term_masks, the shared-anchor rule it is compared with.

Each term Z of a metric has its own record: its value when last computed and the pose it was computed at.  The rule drops Y when
cd_X + d_X + d_Y + margin < cd_Y, d_Z = rho(R, R_Z) * radius + |T - T_Z| and rho = ||R - R_Z||_F / sqrt(2) + the orthogonality
defects of both matrices.  Soundness is checked against float64 numpy with the construction of tests/test_term_masks_host.py:
random clouds of 64..128 points, random poses, small motions sized around the gap between the two directions (so the draws
straddle the threshold) -- here with one record pose per term: whenever the rule drops a term, that term truly loses the min at
the current pose.  The rule sees what the kernel would give it: fp32 poses, fp32 roundings of the recorded terms, an fp32 radius."""
import numpy as np
import pytest

from tests import termanchors
from tests.test_term_masks_host import _rot, _terms

CLOUDS, MOTIONS = 1280, 8           # 10,240 draws
BATCH = 64
_F32 = lambda a: np.asarray(a).astype(np.float32).astype(np.float64)          # noqa: E731


def _clouds(rng):
    """tests/test_term_masks_host.py's clouds: a target that is a cropped, noisy copy of the source plus clutter."""
    n_pts = int(rng.integers(64, 129))
    src = _F32(rng.standard_normal((BATCH, n_pts, 3))) * 0.4
    src = _F32(src)
    keep = int(n_pts * rng.uniform(0.5, 1.0))
    tgt = src.copy()
    tgt[:, keep:] = rng.standard_normal((BATCH, n_pts - keep, 3)) * rng.uniform(0.2, 1.0)
    tgt = _F32(tgt + rng.standard_normal(tgt.shape) * 0.01)
    return src, tgt, np.sqrt((src ** 2).sum(-1).max(1))


def _step(rng, R0, T0, d, radius, rot_div=1.0):
    """A pose at most d away from (R0, T0) (angle * radius + |dT| <= d), rounded to fp32.  rot_div = sqrt(2): at most d in
    term_masks' Frobenius measure, the draws of tests/test_term_masks_host.py."""
    share = rng.uniform(0.0, 1.0, BATCH)                                     # of d spent on the rotation
    dR = _rot(rng.standard_normal((BATCH, 3)), share * d / (rot_div * radius))
    dT = rng.standard_normal((BATCH, 3))
    dT *= ((1.0 - share) * d / np.linalg.norm(dT, axis=1))[:, None]
    return _F32(dR @ R0), _F32(T0 + dT)


def _draws(seed, same_anchor):
    """Yields (cd_rec [b,4,2] float64 of the fp32-rounded records, need_new, need_old, cd_now [b,4,2]).  same_anchor: both
    records of every metric sit at one pose (term_masks' situation)."""
    rng = np.random.default_rng(seed)
    for _ in range(0, CLOUDS, BATCH):
        src, tgt, radius = _clouds(rng)
        Rf = _F32(_rot(rng.standard_normal((BATCH, 3)), rng.uniform(0, np.pi, BATCH)))
        Tf = _F32(rng.uniform(-0.25, 0.25, (BATCH, 3)))
        cd_f = _terms(src, tgt, Rf, Tf)
        gap = np.abs(cd_f[:, :, 0] - cd_f[:, :, 1])                          # [b, 4]
        for _ in range(MOTIONS):
            g = gap[np.arange(BATCH), rng.integers(0, 4, BATCH)]             # motions sized to a random metric's gap
            if same_anchor:
                stale_bits = np.zeros(BATCH, np.int64)
                Rs, Ts = np.repeat(Rf[:, None], 4, 1), np.repeat(Tf[:, None], 4, 1)
                cd_rec = cd_f.copy()
                # as tests/test_term_masks_host.py: 2 d between 0 and 2.5 gaps
                R, T = _step(rng, Rf, Tf, rng.uniform(0.0, 1.25, BATCH) * g * 0.5, radius, np.sqrt(2.0))
            else:
                # one stale term per metric, at its own pose: up to 1.25 gaps from the fresh pose; the current pose up to
                # 1.25 gaps from the fresh one as well (so up to 2.5 from the stale ones): d_X + d_Y straddles the gaps
                stale_dir = rng.integers(0, 2, (BATCH, 4))
                stale_bits = (((stale_dir == 0) * (1 << np.arange(4))) + ((stale_dir == 1) * (16 << np.arange(4)))).sum(1)
                Rs, Ts = np.empty((BATCH, 4, 3, 3)), np.empty((BATCH, 4, 3))
                cd_rec = cd_f.copy()
                for m in range(4):
                    Rs[:, m], Ts[:, m] = _step(rng, Rf, Tf, rng.uniform(0.0, 1.25, BATCH) * g, radius)
                    cd_s = _terms(src, tgt, Rs[:, m], Ts[:, m])
                    rows = np.arange(BATCH)
                    cd_rec[rows, m, stale_dir[:, m]] = cd_s[rows, m, stale_dir[:, m]]
                R, T = _step(rng, Rf, Tf, rng.uniform(0.0, 1.25, BATCH) * g, radius)
            rec = termanchors.records(cd_rec, Rf, Tf, Rs, Ts, stale_bits, R, T, radius)
            new, old = termanchors.run(rec)
            yield _F32(cd_rec), new, old, _terms(src, tgt, R, T)


def _check_sound(need, cd_now, counts):
    for m in range(4):
        need0, need1 = (need >> m) & 1, (need >> (4 + m)) & 1
        assert ((need0 | need1) == 1).all()                                  # never both
        lose0, lose1 = need0 == 0, need1 == 0
        assert (cd_now[lose0, m, 0] > cd_now[lose0, m, 1]).all(), "dropped dir 0 although it wins or ties"
        assert (cd_now[lose1, m, 1] > cd_now[lose1, m, 0]).all(), "dropped dir 1 although it wins or ties"
        counts["dropped"] += int(lose0.sum() + lose1.sum())
    any_drop = (need != 0xFF)
    counts["draws_with_drop"] += int(any_drop.sum())


def test_a_dropped_term_truly_loses_with_one_record_pose_per_term():
    counts = {"dropped": 0, "draws_with_drop": 0}
    draws = draws_keeping_a_gap = 0
    for cd_rec, new, _, cd_now in _draws(2025, same_anchor=False):
        _check_sound(new, cd_now, counts)
        gap = cd_rec[:, :, 0] != cd_rec[:, :, 1]
        kept_both = np.stack([((new >> m) & 1) & ((new >> (4 + m)) & 1) for m in range(4)], 1) == 1
        draws_keeping_a_gap += int((kept_both & gap).any(1).sum())
        draws += len(new)
    assert draws >= 10000
    # not vacuous, and the draws straddle the threshold: at least a tenth of the draws drop a term, at least a tenth keep both
    # terms of a metric whose recorded gap is not zero
    print(f"{draws} draws: {counts['draws_with_drop']} drop a term ({counts['dropped']} terms), {draws_keeping_a_gap} keep both "
          "terms of a metric with a gap")
    assert counts["draws_with_drop"] * 10 >= draws and draws_keeping_a_gap * 10 >= draws, (counts, draws_keeping_a_gap, draws)


def test_with_one_anchor_the_new_rule_drops_whatever_term_masks_drops():
    counts = {"dropped": 0, "draws_with_drop": 0}
    old_dropped = new_only = draws = 0
    for _, new, old, cd_now in _draws(2024, same_anchor=True):
        _check_sound(new, cd_now, counts)
        assert ((new & ~old) == 0).all(), "the new rule keeps a term that term_masks drops"
        old_dropped += int(sum(((old >> b) & 1 == 0).sum() for b in range(8)))
        new_only += int(sum((((old >> b) & 1 == 1) & ((new >> b) & 1 == 0)).sum() for b in range(8)))
        draws += len(new)
    print(f"{draws} draws: term_masks drops {old_dropped} terms, the new rule {new_only} more")
    assert draws >= 10000 and old_dropped > draws * 4 // 10 and new_only > 0


def _spectral(A):
    return np.linalg.svd(A, compute_uv=False)[..., 0]


def _rule_rho_is_sound(Rz, R, radius=1.0):
    """With T = T_Z = 0 and cd = (0, c): dir 1 is dropped iff 2 rho radius (1 + rel) + margins + rel c < c.  Find by bisection the
    smallest c the rule drops at and check it against float64 ||R - R_Z||_2 by SVD: the rule's rho is never below it."""
    n = R.shape[0]
    spec = _spectral(R.astype(np.float64) - Rz.astype(np.float64))
    z3 = np.zeros((n, 3))
    lo, hi = np.zeros(n), np.full(n, 64.0)
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        cd = np.zeros((n, 4, 2))
        cd[:, :, 1] = mid[:, None]
        rec = termanchors.records(cd, Rz, z3, np.repeat(Rz[:, None], 4, 1), np.repeat(z3[:, None], 4, 1), np.zeros(n), R, z3,
                                  np.full(n, radius))
        new, _ = termanchors.run(rec)
        drops = ((new >> 4) & 1) == 0
        hi = np.where(drops, mid, hi)
        lo = np.where(drops, lo, mid)
    # at the threshold c = 2 rho radius (1 + rel) + rel c + abs + move_err * 2 radius  =>  rho from c; the rule's own slack
    # constants only make hi larger, so  hi >= 2 * spec * radius  must hold with them ignored
    assert (hi >= 2.0 * spec * radius).all(), (hi - 2.0 * spec * radius).min()
    return hi, spec


def test_the_sqrt2_bound_with_its_defect_term_is_sound_for_fp32_rotations():
    rng = np.random.default_rng(7)
    n = 4096
    angles = np.exp(rng.uniform(np.log(1e-4), np.log(np.pi), n))
    angles[:8] = [1e-4, 1e-3, 1e-2, 0.1, 1.0, np.pi / 3, 3.0, np.pi]
    Rz = _rot(rng.standard_normal((n, 3)), rng.uniform(0, np.pi, n))
    R = _rot(rng.standard_normal((n, 3)), angles) @ Rz
    Rz32, R32 = Rz.astype(np.float32), R.astype(np.float32)                  # fp32-rounded: no longer exact rotations
    hi, spec = _rule_rho_is_sound(Rz32, R32)
    # and the bound is the tight one where it applies: below 60 degrees rho is within 1e-5 of spec, not 1.41 x spec
    small = (angles < 1.0) & (angles > 1e-2)
    rho = (hi * (1 - 1e-3) - 1e-6 - 2e-6) / (2.0 * (1 + 1e-3))
    assert (rho[small] <= spec[small] * 1.01 + 1e-5).all()
    # poses that differ by one ulp in one entry
    one = R32.copy()
    idx = rng.integers(0, 9, n)
    flat = one.reshape(n, 9)
    flat[np.arange(n), idx] = np.nextafter(flat[np.arange(n), idx], np.float32(2.0))
    _rule_rho_is_sound(R32, one)
    # matrices that are no rotations at all (a reflection, a scaled rotation, a sheared one) fall back to the Frobenius norm
    bad = R32.copy()
    bad[0::3] = bad[0::3] @ np.diag([1.0, 1.0, -1.0]).astype(np.float32)
    bad[1::3] *= np.float32(1.01)
    bad[2::3, 0, 1] += np.float32(0.02)
    _rule_rho_is_sound(Rz32, bad)
    _rule_rho_is_sound(bad, Rz32)


def _one(cd, fresh=None, stale=None, stale_bits=0, R=None, T=None, radius=1.0, nmet=4):
    """fresh / stale[m]: (R, T) or None for the identity pose."""
    eye, zero = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
    fR, fT = (eye, zero) if fresh is None else fresh
    sR = np.stack([eye if stale is None or stale[m] is None else stale[m][0] for m in range(4)])
    sT = np.stack([zero if stale is None or stale[m] is None else stale[m][1] for m in range(4)])
    R = fR if R is None else R
    T = fT if T is None else T
    rec = termanchors.records(np.asarray(cd, np.float64).reshape(1, 4, 2), fR[None], fT[None], sR[None], sT[None],
                              np.asarray([stale_bits]), np.asarray(R)[None], np.asarray(T)[None], np.asarray([radius]))
    return int(termanchors.run(rec, nmet)[0][0])


def test_a_clear_gap_drops_the_loser_and_only_the_loser():
    cd = [[0.1, 0.5], [0.5, 0.1], [0.2, 0.2002], [0.3, 0.3]]
    assert _one(cd) == 0xFF & ~(1 << 4) & ~(1 << 1)          # metric 0: dir 1 loses; metric 1: dir 0 loses; 2, 3: too close
    assert _one(cd, nmet=1) == 0x01
    # the current pose is d_X + d_Y = 0.5 away from the records together: more than the gap of 0.4
    assert _one(cd, T=np.array([0.25, 0.0, 0.0], np.float32)) == 0xFF
    # only the stale term of metric 0 is far away (0.45): metric 0 keeps both, metric 1 (both records fresh) still drops
    far = (np.eye(3, dtype=np.float32), np.array([0.45, 0.0, 0.0], np.float32))
    assert _one(cd, stale=[far, far, None, None], stale_bits=0x10) == 0xFF & ~(1 << 1)
    assert _one(cd, stale=[far, far, None, None], stale_bits=0x00) == 0xFF & ~(1 << 4) & ~(1 << 1)   # not marked stale: not used


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf")])
def test_nan_and_inf_keep_both_terms(bad):
    base = [[0.1, 0.5]] * 4
    eye, zero = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
    for d in (0, 1):
        cd = [row[:] for row in base]
        cd[2][d] = bad
        need = _one(cd)
        assert (need >> 2) & 1 and (need >> 6) & 1, hex(need)
        assert need & ~0x44 == 0xFF & ~0x44 & ~0xB0              # the other metrics still drop their dir 1
    Rbad = eye.copy()
    Rbad[1, 1] = bad
    Tbad = np.array([0.0, bad, 0.0], np.float32)
    assert _one(base, R=Rbad) == 0xFF and _one(base, fresh=(Rbad, zero), R=eye) == 0xFF
    assert _one(base, T=Tbad) == 0xFF and _one(base, fresh=(eye, Tbad), T=zero) == 0xFF
    assert _one(base, fresh=(Rbad, zero), R=Rbad) == 0xFF and _one(base, fresh=(eye, Tbad), T=Tbad) == 0xFF
    # a bad entry in the stale pose of metric 1 keeps both terms of metric 1, whichever term is the stale one
    for bits in (0x02, 0x20):
        for pose in ((Rbad, zero), (eye, Tbad)):
            need = _one(base, stale=[None, pose, None, None], stale_bits=bits)
            assert need == 0xFF & ~0xD0, hex(need)
    assert _one(base, radius=bad) == 0xFF                    # 0 * inf included: the pose has not moved
    assert _one(base, radius=bad, T=np.array([0.01, 0.0, 0.0], np.float32)) == 0xFF


def test_ties_keep_both_terms():
    assert _one([[0.25, 0.25]] * 4) == 0xFF
    assert _one([[0.0, 0.0]] * 4) == 0xFF
    one_ulp = np.nextafter(np.float32(0.25), np.float32(1))
    assert _one([[0.25, one_ulp], [one_ulp, 0.25], [0.25, 0.25], [0.25, 0.25]]) == 0xFF
