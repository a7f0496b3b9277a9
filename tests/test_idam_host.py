"""CPU: the NumPy restatement of the IDAM contracts (tests/idam_host.py) is consistent with itself and with the bounds of
tests/idam_cases.py, and houv_amd.models.idam.Model carries the reference's state_dict names (tests/golden/idam_weights.py
lists them: that list loads into the reference's registration/models/idam.py Model with nothing unexpected and only the
BatchNorm `num_batches_tracked` counters missing)."""
import os
import sys

import numpy as np

import idam_cases as cases
import idam_host as host

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import idam_weights  # noqa: E402


def test_state_dict_names_equal_the_reference():
    from houv_amd.models.idam import Model
    net = Model(idam_weights.Args)
    own = {k: tuple(v.shape) for k, v in net.state_dict().items() if not k.endswith("num_batches_tracked")}
    want = dict(idam_weights.spec())
    want["head.reflect"] = (3, 3)
    assert own == want
    assert "emb_nn.propogate1.conv2d.conv.0.conv.weight" in own and own["sim_mat_conv1.0.conv.0.conv.weight"] == (32, 132, 1, 1)


def test_float32_restatement_is_within_the_bounds():
    """The bounds are 4x what idam_cases.py measured: the float32 restatement itself has to sit inside them, on every small case."""
    for shape in cases.SIM_SHAPES:
        if shape[1] > 65:
            continue                                    # the 341 x 341 case takes seconds in NumPy: `python tests/idam_cases.py` runs it
        case = cases.sim_case(*shape)
        y, flagged = cases.sim_yardstick(case)
        f = host.simmat(*case, dtype=np.float32)
        assert f["scores"].dtype == np.float32 and y["scores"].dtype == np.float64
        cases.check_sim(f["rowmax"], f["scores"], f["corr_idx"], None, case, y, flagged, f"float32 restatement {shape}")
        assert 4 * np.abs(f["scores"] - y["scores"]).max() <= cases.TOL_SCORE


def test_duplicated_targets_and_coincident_points():
    case = cases.sim_case(2, 16, 16, 64)
    y = host.simmat(*case, dtype=np.float64)
    assert np.isfinite(y["scores"]).all()
    assert np.array_equal(y["scores"][..., 1], y["scores"][..., 2]) and np.array_equal(y["scores"][..., 1], y["scores"][..., 14])
    assert not np.isin(y["corr_idx"], [2, 14]).any()    # the lowest j among equal scores


def test_flagged_rows_rule():
    s = np.array([[20.0, 20.0, 19.99999, 3.0],           # 20 and 19.99999: closer than the bound, not both +-20 -> flagged
                  [20.0, 20.0, 5.0, -20.0],              # 20 and 5 -> not flagged
                  [-20.0, -20.0, -20.0, -20.0],          # a single distinct value -> not flagged
                  [20.0, -20.0, -20.0, -20.0],           # both exactly +-20 -> not flagged
                  [1.0, 1.00001, 0.0, 0.0]])             # closer than the bound -> flagged
    assert host.flagged_rows(s, 1e-4).tolist() == [True, False, False, False, True]


def test_edge_diff_restatement():
    x, idx = cases.edge_case(1, 12, 12, 3)
    out = host.edge_diff(x, idx, 12, 4).reshape(1, 12, 12, 4)
    assert (out[..., 3] == 0).all() and (out[:, :, 0, :] == 0).all()
    assert np.array_equal(out[0, 0, 1, :3], x[0, 0] - x[0, 0]) and np.array_equal(out[0, 11, 11, :3], x[0, 11] - x[0, 11])
    assert np.array_equal(out[0, 5, 3, :3], x[0, idx[0, 5, 3]] - x[0, 5])


# ---------------------------------------------------------------------------------------------------------------- the reference
G24_CASES = ("n96", "n192", "n768")


def _err(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)).max())


def test_restatement_reproduces_the_reference_in_float32(golden):
    """tests/golden/g24_idam.npz holds a float32 forward of the REAL registration/models/idam.py.  The float32 restatement
    reproduces it from the stored inputs and weights, every iteration from the reference's own inputs of that iteration:
    embeddings, significance, rowmax, scores, weights, R, t within 4x the fixture's own float32-vs-float64 spread of the
    restatement (R and t: the case's own spread), the kept sets exactly (and the lists in order wherever the reference's order is
    the restatement's float64 order too), corr_idx exactly on unflagged rows."""
    g = golden("g24_idam.npz")
    state = idam_weights.make_state()
    bound = 4 * float(g["spread_scores"])
    for name in G24_CASES:
        src, tgt = g[f"{name}_src"], g[f"{name}_tgt"]
        B, N, _ = src.shape
        bi = np.arange(B)[:, None]
        for c, cloud in (("src", src), ("tgt", tgt)):
            emb = host.embed(state, cloud, g[f"{name}_knn_{c}"], np.float32)
            sig = host.significance(state, emb, np.float32)
            kept = g[f"{name}_{c}_idx"]
            e_emb, e_sig = _err(emb[bi, kept], g[f"{name}_e{c[0]}"]), _err(sig, g[f"{name}_sig_{c}"])
            print(name, c, "embedding", e_emb, "bound", 4 * float(g["spread_emb"]), "significance", e_sig, "bound", 4 * float(g["spread_sig"]))
            assert e_emb <= 4 * float(g["spread_emb"]) and e_sig <= 4 * float(g["spread_sig"])
            own = host.keep(sig, N // 6)
            assert np.array_equal(np.sort(own, -1), np.sort(kept, -1))
            own64 = host.keep(host.significance(state, host.embed(state, cloud, g[f"{name}_knn_{c}"], np.float64), np.float64), N // 6)
            if np.array_equal(own64, kept):
                assert np.array_equal(own, kept)
        src_at = [g[f"{name}_src_at{i}"] for i in range(idam_weights.NUM_ITERS)]
        tk = tgt[bi, g[f"{name}_tgt_idx"]]
        its, T = host.stepwise(state, src_at, tk, g[f"{name}_es"], g[f"{name}_et"], np.float32)
        y64, _ = host.stepwise(state, src_at, tk, g[f"{name}_es"], g[f"{name}_et"], np.float64)
        for i, (it, y) in enumerate(zip(its, y64)):
            flagged = host.flagged_rows(y["scores"], bound)
            assert flagged.mean() <= 0.02
            for q, spread in (("rowmax", g["spread_rowmax"]), ("scores", g["spread_scores"]), ("weights", g["spread_weights"]),
                              ("R", g[f"{name}_spread_R"]), ("t", g[f"{name}_spread_t"])):
                e = _err(it[q], g[f"{name}_{q}{i}"])
                print(name, "iteration", i, q, e, "bound", 4 * float(spread))
                assert e <= 4 * float(spread), (name, i, q)
            assert np.array_equal(it["corr_idx"][~flagged], g[f"{name}_corr_idx{i}"][~flagged])
            assert np.array_equal(y["corr_idx"][~flagged], g[f"{name}_corr_idx{i}"][~flagged])
        e = _err(host.compose([g[f"{name}_R{i}"] for i in range(3)], [g[f"{name}_t{i}"] for i in range(3)], np.float64), g[f"{name}_T"])
        print(name, "T of the reference against the composition of its own iterations", e)
        assert e <= 1e-5                                  # the fixture is consistent with itself: compose() is the reference's rule
        assert np.array_equal(g[f"{name}_T"][:, 3], np.broadcast_to(np.float32([0, 0, 0, 1]), (B, 4)))


def test_state_dict_key_list_equals_the_stored_one(golden):
    from houv_amd.models.idam import Model
    g = golden("g24_idam.npz")
    net = Model(idam_weights.Args)
    assert sorted(k for k in net.state_dict() if not k.endswith("num_batches_tracked")) == [str(k) for k in g["state_keys"]]
