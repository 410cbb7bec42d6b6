"""The data-set preparation of the network trainers (radar_ml_amd.prep, dnn.preprocess_data, sgan.preprocess_data) without a GPU: the
NumPy twin of tests/prep_common.py reproduces the reference's recorded run (tests/golden/prep_golden.npz) bit for bit, the package's
host half makes the reference's draws in the reference's order, and the library exports the chain."""
import ctypes

import numpy as np
import pytest

import prep_common as pc


@pytest.fixture(scope="module")
def tw():
    return pc.twin_runs()


def test_twin_reproduces_every_stage_plane_of_the_reference(tw):
    g = tw["g"]
    for k in range(pc.SETTINGS):
        want = g["stage_digest%d" % k]
        for i in range(len(tw["data"])):
            for pi in range(3):
                for st in range(3):
                    assert pc.digest(tw["stage"][k][i][pi][st + 1]) == want[i, pi, st], (k, i, pi, pc.STAGES[st])
    # the planes stored in full say the same, and show the digests are of what they claim to be
    for key in g.files:
        if key.startswith("stage") and key[5].isdigit() and "_" in key:
            k, i, pi = (int(v) for v in key[5:].split("_"))
            np.testing.assert_array_equal(np.stack(tw["stage"][k][i][pi][1:]), g[key])
    for i in range(len(tw["data"])):
        for pi in range(3):
            assert pc.digest(tw["resized1"][i][pi]) == g["resized_digest1"][i, pi]


def test_golden_meets_its_conditions(tw):
    g = tw["g"]
    zooms = np.concatenate([g["zoom0"], g["zoom1"]])
    assert (zooms < 1.0).any() and (zooms > 1.0).any()
    final = np.concatenate([tw["stage"][1][i][pi][3].ravel() for i in range(9) for pi in range(3)])
    assert np.mean((final > -1.0) & (final < 1.0)) >= 0.5          # a saturated plane would hide every error
    # corners leave the plane at 15 degrees: the rotated Walabot planes hold exact zeros (cval) in the [-1, 1] domain
    assert (tw["stage"][1][0][0][1] == 0.0).any()
    assert sorted(np.bincount(np.unique(g["labels"], return_inverse=True)[1])) == [1, 3, 5]


@pytest.mark.parametrize("mod", ["dnn", "sgan"])
@pytest.mark.parametrize("aug", [0, 1])
def test_twin_reproduces_preprocess_data(tw, mod, aug):
    g, run, key = tw["g"], tw["runs"][(mod, aug)], "%s_%d_" % (mod, aug)
    np.testing.assert_array_equal(run["order"], g[key + "order"])
    assert run["n_classes"] == int(g[key + "n_classes"]) == 3
    np.testing.assert_array_equal(run["w_keys"], g[key + "w_keys"])
    np.testing.assert_array_equal(run["w_vals"], g[key + "w_vals"])
    np.testing.assert_array_equal(run["y_val"], g[key + "y_val"])
    assert pc.digest(run["X_val"]) == str(g[key + "X_val"])
    if mod == "dnn":
        np.testing.assert_array_equal(run["y_train"], g[key + "y_train"])
        assert pc.digest(run["X_train"]) == str(g[key + "X_train"])
        assert run["X_train"].shape == (7, 80, 80, 3) and run["X_val"].shape == (2, 80, 80, 3)
    else:
        np.testing.assert_array_equal(run["y_bal"], g[key + "y_bal"])
        np.testing.assert_array_equal(run["sup_bal"], g[key + "sup_bal"])
        assert pc.digest(run["X_bal"]) == str(g[key + "X_bal"])            # hence the balance indices
        assert len(set(np.bincount(run["y_bal"]).tolist()) - {0}) == 1 and run["X_bal"].shape[1:] == (128, 128, 3)
    if aug:
        np.testing.assert_array_equal(run["angles"], g["angles0"])
        np.testing.assert_array_equal(run["zoom"], g["zoom0"])
        np.testing.assert_array_equal(run["noise"], g["noise0"])


@pytest.mark.parametrize("mod", ["dnn", "sgan"])
@pytest.mark.parametrize("aug", [0, 1])
def test_host_plan_makes_the_reference_draws_in_order(rml, tw, mod, aug):
    from radar_ml_amd import prep
    g, key = tw["g"], "%s_%d_" % (mod, aug)
    np.random.seed(int(g["np_seed0"]))
    rng = np.random.default_rng(1234)
    plan = prep.plan_dataset(pc.Args(bool(aug)), 9, 3, tw["labels"], rng, samples_sup=tw["sup"] if mod == "sgan" else None, balance=mod == "sgan")
    np.testing.assert_array_equal(plan.order, g[key + "order"])
    assert plan.split == 7 and plan.n_classes == 3
    assert {int(k): v for k, v in plan.w_classes.items()} == dict(zip(g[key + "w_keys"].tolist(), g[key + "w_vals"].tolist()))
    y = plan.labels[plan.order]
    np.testing.assert_array_equal(y[7:], g[key + "y_val"])
    if aug:
        np.testing.assert_array_equal(plan.draws.angles, g["angles0"])
        np.testing.assert_array_equal(plan.draws.zoom, g["zoom0"])
        np.testing.assert_array_equal(plan.draws.noise, g["noise0"])
        assert plan.draws.stages == 7
    else:
        assert plan.draws is None
    if mod == "sgan":
        np.testing.assert_array_equal(plan.balance, tw["runs"][(mod, aug)]["bal_idx"])
        np.testing.assert_array_equal(y[:7][plan.balance], g[key + "y_bal"])
        np.testing.assert_array_equal(tw["sup"][plan.order][:7][plan.balance], g[key + "sup_bal"])
    else:
        assert plan.balance is None
        np.testing.assert_array_equal(y[:7], g[key + "y_train"])
    # what comes next on both sources is what came next for the twin: nothing more, nothing less was drawn
    np.random.seed(int(g["np_seed0"]))
    rng2 = np.random.default_rng(1234)
    pc.preprocess(pc.Args(bool(aug)), [(np.zeros((2, 2), np.float32),) * 3] * 9, tw["labels"], (4, 4), rng2, tw["sup"] if mod == "sgan" else None)
    after_twin = (np.random.uniform(), rng2.random())
    np.random.seed(int(g["np_seed0"]))
    rng3 = np.random.default_rng(1234)
    prep.plan_dataset(pc.Args(bool(aug)), 9, 3, tw["labels"], rng3, samples_sup=tw["sup"] if mod == "sgan" else None, balance=mod == "sgan")
    assert (np.random.uniform(), rng3.random()) == after_twin


def test_second_setting_draws_and_chain_parameters(rml, tw):
    from radar_ml_amd import prep
    g = tw["g"]
    rot, zr, sd = g["setting1"]
    np.random.seed(int(g["np_seed1"]))
    d = prep.draw_augment(9, 3, float(rot), float(zr), float(sd), np.random.default_rng(1234))
    np.testing.assert_array_equal(d.angles, g["angles1"])
    np.testing.assert_array_equal(d.zoom, g["zoom1"])
    np.testing.assert_array_equal(d.noise, g["noise1"])
    par = d.params([2, 5], 1, (31, 176))
    assert par.shape == (2, 8) and par.dtype == np.float64
    np.testing.assert_array_equal(par[:, 6], g["zoom1"][[2, 5]])
    np.testing.assert_array_equal(par[:, 7], g["noise1"][[2, 5], 1])
    np.testing.assert_array_equal(par[1, :6], rml.rotation_params(g["angles1"][5, 1], (31, 176)))


def test_a_none_stage_skips_its_draws(rml):
    from radar_ml_amd import prep, _lib

    def after(rot, zr, sd):
        np.random.seed(5)
        rng = np.random.default_rng(6)
        d = prep.draw_augment(2, 3, rot, zr, sd, rng)
        return d, np.random.uniform(), rng.random()

    np.random.seed(5)
    u = [np.random.uniform() for _ in range(9)]
    n = np.random.default_rng(6)
    nn = [n.normal() for _ in range(6)] + [n.random()]
    d, nu, nr = after(None, None, None)
    assert d.stages == 0 and d.angles is None and d.zoom is None and d.noise is None and nu == u[0]
    assert nr == np.random.default_rng(6).random()
    d, nu, nr = after(1.0, None, None)
    assert d.stages == _lib.CHAIN_ROTATE and nu == u[6] and nr == np.random.default_rng(6).random()
    d, nu, nr = after(None, 0.3, None)
    assert d.stages == _lib.CHAIN_ZOOM and nu == u[2] and d.zoom.shape == (2,)
    d, nu, nr = after(None, None, 1.0)
    assert d.stages == _lib.CHAIN_NOISE and nu == u[0] and nr == nn[6]
    np.testing.assert_array_equal(d.noise.ravel(), nn[:6])
    d, nu, nr = after(1.0, 0.3, 1.0)
    assert d.stages == 7 and nu == u[8] and nr == nn[6]
    assert d.params([0, 1], 0, (5, 7))[:, 6].tolist() == d.zoom.tolist()


def test_balance_classes_on_a_balanced_set_returns_its_input(rml):
    from radar_ml_amd import sgan
    data, labels, sup = np.arange(24.0).reshape(6, 4), np.array([2, 0, 1, 1, 0, 2]), np.array([True] * 6)
    rng = np.random.default_rng(3)
    out = sgan.balance_classes(data, labels, sup, rng=rng)
    assert out[0] is data and out[1] is labels and out[2] is sup
    assert rng.random() == np.random.default_rng(3).random()            # and draws nothing
    # an imbalanced host set: every class gets the largest class's size, rows keep their labels and masks
    labels = np.array([0, 0, 0, 1, 1, 2])
    sup = np.array([True, False, True, False, True, True])
    d, l, s = sgan.balance_classes(data, labels, sup, rng=np.random.default_rng(3))
    assert np.bincount(l).tolist() == [3, 3, 3]
    rows = (d[:, 0] // 4).astype(int)
    np.testing.assert_array_equal(labels[rows], l)
    np.testing.assert_array_equal(sup[rows], s)
    np.testing.assert_array_equal(rows, pc.balance_picks(labels, np.random.default_rng(3)))
    d2, l2, _ = sgan.balance_classes(data, labels, sup, shuffle=False)
    assert l2.tolist() == [0, 0, 0, 1, 1, 1, 2, 2, 2]


def test_an_empty_validation_split_is_planned_as_the_reference_does(rml, tw):
    from radar_ml_amd import prep
    plan = prep.plan_dataset(pc.Args(False, 1.0), 9, 3, tw["labels"], np.random.default_rng(1234), samples_sup=tw["sup"], balance=True)
    assert plan.split == 9 and plan.balance is not None and len(plan.balance) == 15
    twin = pc.preprocess(pc.Args(False, 1.0), [(np.zeros((2, 2), np.float32),) * 3] * 9, tw["labels"], (4, 4), np.random.default_rng(1234), tw["sup"])
    np.testing.assert_array_equal(plan.balance, twin["bal_idx"])
    # the package's rule (sgan.py:722-723) sits in the plan: the validation set is the training part before balancing -- all nine rows in
    # shuffled order, not the 15 balanced ones and not an empty array; dnn.py has no such rule, and a real split does not trigger it
    assert plan.val_is_train is True and twin["val_is_train"]
    np.testing.assert_array_equal(plan.labels[plan.order][:plan.split], twin["y_val"])
    assert len(twin["y_val"]) == 9 and len(twin["y_bal"]) == 15
    assert prep.plan_dataset(pc.Args(False, 1.0), 9, 3, tw["labels"], np.random.default_rng(1234)).val_is_train is False
    assert prep.plan_dataset(pc.Args(False, 0.8), 9, 3, tw["labels"], np.random.default_rng(1234), samples_sup=tw["sup"], balance=True).val_is_train is False
    with pytest.raises(ValueError, match="empty data set"):
        prep.plan_dataset(pc.Args(False, 0.8), 0, 0, [], np.random.default_rng(0))
    # a split beyond 1 is capped at the data set
    assert prep.plan_dataset(pc.Args(False, 1.5), 9, 3, tw["labels"], np.random.default_rng(0)).split == 9


def test_front_doors_have_the_reference_signatures(rml):
    import inspect
    from radar_ml_amd import dnn, sgan
    for mod in (dnn, sgan):
        sig = inspect.signature(mod.augment_data)
        assert list(sig.parameters)[:5] == ["x", "rotation_range", "zoom_range", "noise_sd", "rng"]
        assert [sig.parameters[k].default for k in ("rotation_range", "zoom_range", "noise_sd", "rng")] == [1.0, 0.3, 1.0, None]
        assert isinstance(mod.rng, np.random.Generator)            # the module-level default_rng(1234) of the reference
    assert list(inspect.signature(dnn.preprocess_data).parameters) == ["args", "data", "labels", "rng", "device", "return_numpy"]
    assert list(inspect.signature(sgan.preprocess_data).parameters) == ["args", "data", "labels", "samples_sup", "rng", "device", "return_numpy"]
    assert list(inspect.signature(sgan.balance_classes).parameters) == ["data", "labels", "samples_sup", "shuffle", "rng"]
    assert dnn.RESCALE == (80, 80) and sgan.RESCALE == (128, 128)


def test_library_exports_the_chain(built_lib):
    lib = ctypes.CDLL(built_lib)
    assert hasattr(lib, "rml_augment_chain"), "libradarml_hip.so does not export rml_augment_chain"
    from radar_ml_amd import _lib
    assert "rml_augment_chain" in _lib.SIGNATURES and len(_lib.SIGNATURES["rml_augment_chain"][1]) == 14
    assert (_lib.CHAIN_ROTATE, _lib.CHAIN_ZOOM, _lib.CHAIN_NOISE) == (1, 2, 4)
