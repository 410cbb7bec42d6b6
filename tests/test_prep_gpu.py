"""The data-set preparation of the network trainers on the GPU: ``rml_augment_chain`` (csrc/augment_chain.hip) stage by stage and as one
launch, ``dnn.preprocess_data`` / ``sgan.preprocess_data`` and the device-resident hand-over to ``Classifier.fit``, against the
reference's recorded run (tests/golden/prep_golden.npz).  The expected arrays are those of the NumPy twin (tests/prep_common.py), which
test_prep_cpu.py shows to equal the reference's bit for bit -- the large ones are in the golden as digests, checked here again.

Bounds.  One spline stage (rotate, zoom): 4e-6 absolute -- the project's 2e-6 on [0, 1] for one stage
(test_augmentation_kernels_match_the_reference_data_generator), doubled for the doubled range [-1, 1].  The whole chain, and the chain
followed by the resize: 1.2e-5, three stage bounds: a one-ulp perturbation after the rotation is still one ulp (1.2e-7) after the
reference's zoom and two (2.4e-7) after its resize, so the stages add and do not amplify.  Scaling, noise + clamp, the resize itself, every
gather: bit-exact.  Worst deviations measured on an MI355X are in DESIGN.md 3.5d."""
import numpy as np
import pytest

import prep_common as pc

pytestmark = pytest.mark.gpu
STAGE_TOL = 4e-6
CHAIN_TOL = 1.2e-5


@pytest.fixture(scope="module")
def tw():
    return pc.twin_runs()


@pytest.fixture(scope="module")
def P(rml):
    from radar_ml_amd import prep
    return prep


def by_shape(data):
    """{(projection, shape): sample rows}"""
    groups = {}
    for i, s in enumerate(data):
        for pi, p in enumerate(s):
            groups.setdefault((pi, p.shape), []).append(i)
    return groups


def params(rml, g, k, rows, pi, shape):
    par = np.zeros((len(rows), 8))
    par[:, :6] = [rml.rotation_params(g["angles%d" % k][i, pi], shape) for i in rows]
    par[:, 6] = g["zoom%d" % k][rows]
    par[:, 7] = g["noise%d" % k][rows, pi]
    return par


def test_scaling_is_numpy_float32(rml, P, tw):
    from radar_ml_amd import _lib
    for (pi, shape), rows in by_shape(tw["data"]).items():
        raw = np.stack([tw["data"][i][pi] for i in rows])
        got = P.chain_planes(raw, 0, sub=127.5, div=127.5).cpu().numpy()
        np.testing.assert_array_equal(got, np.stack([pc.scale(p) for p in raw]))
        np.testing.assert_array_equal(P.chain_planes(raw, 0).cpu().numpy(), raw)            # div == 0: the planes themselves
        # the scaling in front of a stage is the same scaling: noise alone, from raw planes
        par = params(rml, tw["g"], 1, rows, pi, shape)
        got = P.chain_planes(raw, _lib.CHAIN_NOISE, par, sub=127.5, div=127.5).cpu().numpy()
        np.testing.assert_array_equal(got, np.stack([pc.add_noise(pc.scale(p), par[j, 7]) for j, p in enumerate(raw)]))


@pytest.mark.parametrize("k", range(pc.SETTINGS))
def test_each_stage_alone_from_the_previous_stage_plane(rml, P, tw, k):
    from radar_ml_amd import _lib
    g, worst = tw["g"], [0.0, 0.0, 0.0]
    for i in range(9):          # the twin's planes are the reference's
        for pi in range(3):
            assert [pc.digest(a) for a in tw["stage"][k][i][pi][1:]] == g["stage_digest%d" % k][i, pi].tolist()
    for (pi, shape), rows in by_shape(tw["data"]).items():
        par = params(rml, g, k, rows, pi, shape)
        for st, mask in enumerate((_lib.CHAIN_ROTATE, _lib.CHAIN_ZOOM, _lib.CHAIN_NOISE)):
            src = np.stack([tw["stage"][k][i][pi][st] for i in rows])
            want = np.stack([tw["stage"][k][i][pi][st + 1] for i in rows])
            got = P.chain_planes(src, mask, par).cpu().numpy()
            worst[st] = max(worst[st], float(np.abs(got - want).max()))
            if st == 2:
                np.testing.assert_array_equal(got, want)
            else:
                assert np.abs(got - want).max() <= STAGE_TOL, (pc.STAGES[st], pi, shape, np.abs(got - want).max())
    print("setting %d: worst deviation rotate %.3g, zoom %.3g, noise %.3g" % (k, *worst))


def test_zoom_factor_one_and_mixed_factors(P, tw):
    from radar_ml_amd import _lib
    worst = 0.0
    for (pi, shape), rows in by_shape(tw["data"]).items():
        src = np.stack([tw["stage"][1][i][pi][1] for i in rows])
        src = np.concatenate([src, src])[:6] if len(src) >= 3 else src
        factors = np.array([0.7, 1.0, 1.3, 0.85, 1.0, 1.17])[:len(src)]
        par = np.zeros((len(src), 8))
        par[:, 6] = factors
        got = P.chain_planes(src, _lib.CHAIN_ZOOM, par).cpu().numpy()
        want = np.stack([pc.clipped_zoom(p, f) for p, f in zip(src, factors)])
        worst = max(worst, float(np.abs(got - want).max()))
        assert np.abs(got - want).max() <= STAGE_TOL, (shape, np.abs(got - want).max())
        np.testing.assert_array_equal(got[factors == 1.0], want[factors == 1.0])            # factor 1: the clamped input, bit for bit
    print("mixed zoom factors: worst deviation %.3g" % worst)


@pytest.mark.parametrize("k", range(pc.SETTINGS))
def test_whole_chain_in_one_launch_and_after_the_resize(rml, P, tw, k):
    from radar_ml_amd import _lib
    from radar_ml_amd.nn_common import resize_bicubic
    g, worst, worst_r = tw["g"], 0.0, 0.0
    for (pi, shape), rows in by_shape(tw["data"]).items():
        raw = np.stack([tw["data"][i][pi] for i in rows])
        got_t = P.chain_planes(raw, _lib.CHAIN_ROTATE | _lib.CHAIN_ZOOM | _lib.CHAIN_NOISE, params(rml, g, k, rows, pi, shape), sub=127.5, div=127.5)
        got = got_t.cpu().numpy()
        want = np.stack([tw["stage"][k][i][pi][3] for i in rows])
        worst = max(worst, float(np.abs(got - want).max()))
        assert np.abs(got - want).max() <= CHAIN_TOL, (pi, shape, np.abs(got - want).max())
        assert got.min() >= -1.0 and got.max() <= 1.0
        if k == 1:
            for i in rows:
                assert pc.digest(tw["resized1"][i][pi]) == g["resized_digest1"][i, pi]
            res = resize_bicubic(got_t, (80, 80), scale=False).cpu().numpy()
            want_r = np.stack([tw["resized1"][i][pi] for i in rows])
            worst_r = max(worst_r, float(np.abs(res - want_r).max()))
            assert np.abs(res - want_r).max() <= CHAIN_TOL, (pi, shape, np.abs(res - want_r).max())
    print("setting %d: worst deviation of the chain %.3g, after the resize %.3g" % (k, worst, worst_r))


def run_module(rml, tw, mod, aug, data=None, **kw):
    import radar_ml_amd.dnn as dnn
    import radar_ml_amd.sgan as sgan
    g = tw["g"]
    np.random.seed(int(g["np_seed0"]))
    rng = np.random.default_rng(1234)
    data = tw["data"] if data is None else data
    if mod == "dnn":
        X_train, y_train, X_val, y_val, n, w = dnn.preprocess_data(pc.Args(bool(aug)), data, tw["labels"], rng=rng, **kw)
        return dict(X_train=X_train, y_train=y_train, X_val=X_val, y_val=y_val, n_classes=n, w=w)
    (X, y, sup), (X_val, y_val), n, w = sgan.preprocess_data(pc.Args(bool(aug)), data, tw["labels"], tw["sup"], rng=rng, **kw)
    return dict(X_bal=X, y_bal=y, sup_bal=sup, X_val=X_val, y_val=y_val, n_classes=n, w=w)


@pytest.mark.parametrize("mod", ["dnn", "sgan"])
def test_preprocess_data_without_augment_is_the_reference_bit_for_bit(rml, tw, mod):
    g, want, key = tw["g"], tw["runs"][(mod, 0)], "%s_0_" % mod
    got = run_module(rml, tw, mod, 0)
    for name in ("X_train", "X_bal", "X_val"):
        if name in got:
            assert pc.digest(want[name]) == str(g[key + name])
            assert got[name].dtype == np.float32
            np.testing.assert_array_equal(got[name], want[name])
    for name in ("y_train", "y_bal", "sup_bal", "y_val"):
        if name in got:
            np.testing.assert_array_equal(got[name], g[key + name])
    assert got["n_classes"] == 3
    assert {int(k): v for k, v in got["w"].items()} == dict(zip(g[key + "w_keys"].tolist(), g[key + "w_vals"].tolist()))


@pytest.mark.parametrize("mod", ["dnn", "sgan"])
def test_preprocess_data_with_augment(rml, tw, mod):
    g, want, key = tw["g"], tw["runs"][(mod, 1)], "%s_1_" % mod
    got = run_module(rml, tw, mod, 1)
    for name in ("X_train", "X_bal", "X_val"):
        if name in got:
            assert pc.digest(want[name]) == str(g[key + name])
            assert got[name].shape == want[name].shape
            d = float(np.abs(got[name] - want[name]).max())
            print("%s augment %s: worst deviation %.3g" % (mod, name, d))
            assert d <= CHAIN_TOL
    for name in ("y_train", "y_bal", "sup_bal", "y_val"):
        if name in got:
            np.testing.assert_array_equal(got[name], g[key + name])
    # the same call twice: the same bits; and the tensors of return_numpy=False are these arrays
    again = run_module(rml, tw, mod, 1, return_numpy=False)
    for name in ("X_train", "X_bal", "X_val"):
        if name in got:
            assert again[name].is_cuda and again[name].is_contiguous()
            np.testing.assert_array_equal(again[name].cpu().numpy(), got[name])


def test_empty_validation_split(rml, tw):
    """train_split 1.0: sgan.preprocess_data returns the training part as it was BEFORE balancing as the validation set (sgan.py:722-723)
    beside the balanced training set; dnn.preprocess_data returns an empty validation set (dnn.py:265-267)"""
    import radar_ml_amd.dnn as dnn
    import radar_ml_amd.sgan as sgan
    data, labels, sup = tw["data"], tw["labels"], tw["sup"]
    want = pc.preprocess(pc.Args(False, 1.0), data, labels, (128, 128), np.random.default_rng(1234), sup)
    assert want["val_is_train"] and len(want["y_train"]) == 9 and len(want["y_bal"]) == 15
    for keep in (True, False):
        (X, y, s), (X_val, y_val), n, w = sgan.preprocess_data(pc.Args(False, 1.0), data, labels, sup, rng=np.random.default_rng(1234), return_numpy=keep)
        if not keep:
            assert X.is_cuda and X_val.is_cuda
            X, X_val = X.cpu().numpy(), X_val.cpu().numpy()
        assert X_val.shape == (9, 128, 128, 3) and X.shape == (15, 128, 128, 3) and n == 3
        np.testing.assert_array_equal(X_val, want["X_train"])              # all nine rows, shuffled, not balanced
        np.testing.assert_array_equal(y_val, want["y_train"])
        np.testing.assert_array_equal(X, want["X_bal"])
        np.testing.assert_array_equal(y, want["y_bal"])
        np.testing.assert_array_equal(s, want["sup_bal"])
        assert np.bincount(y).tolist() == [5, 5, 5] and np.bincount(y_val).tolist() != [5, 5, 5]
    want = pc.preprocess(pc.Args(False, 1.0), data, labels, (80, 80), np.random.default_rng(1234))
    X_train, y_train, X_val, y_val, n, w = dnn.preprocess_data(pc.Args(False, 1.0), data, labels, rng=np.random.default_rng(1234))
    assert X_val.shape == (0, 80, 80, 3) and X_val.dtype == np.float32 and y_val.shape == (0,)
    np.testing.assert_array_equal(X_train, want["X_train"])
    np.testing.assert_array_equal(y_train, want["y_train"])
    with pytest.raises(ValueError, match="empty data set"):
        dnn.preprocess_data(pc.Args(False), [], [])


def test_mixed_shape_data_set_lands_at_its_shuffled_positions(rml, tw):
    """Walabot and small planes interleaved in one list: every (projection, shape) group is a scattered set of rows"""
    mix = [0, 6, 1, 7, 2, 8, 3, 4, 5]
    data = [tw["data"][i] for i in mix]
    got = run_module(rml, tw, "dnn", 0, data=data)
    order = tw["g"]["dnn_0_order"]              # the shuffle does not depend on the planes
    X = np.concatenate([got["X_train"], got["X_val"]])
    for j, src in enumerate(order):
        want = np.stack([pc.resize(pc.scale(p), (80, 80)) for p in data[src]], axis=-1)
        np.testing.assert_array_equal(X[j], want)
    labels = np.unique(tw["labels"], return_inverse=True)[1]
    np.testing.assert_array_equal(np.concatenate([got["y_train"], got["y_val"]]), labels[order])


def test_augment_data_front_door(rml, tw):
    import torch
    import radar_ml_amd.dnn as dnn
    import radar_ml_amd.sgan as sgan
    g = tw["g"]
    rot, zr, sd = (float(v) for v in g["setting1"])
    for mod in (dnn, sgan):
        np.random.seed(int(g["np_seed1"]))
        rng = np.random.default_rng(1234)
        for i in (0, 6):
            x = tuple(tw["stage"][1][i][pi][0] for pi in range(3))
            out = mod.augment_data(x, rot, zr, sd, rng=rng) if i == 0 else mod.augment_data(tuple(torch.from_numpy(p).cuda() for p in x), rot, zr, sd, rng=rng)
            for pi in range(3):
                o = out[pi] if i == 0 else out[pi].cpu().numpy()
                assert (isinstance(out[pi], np.ndarray) if i == 0 else out[pi].is_cuda) and o.dtype == np.float32
                want = tw["stage"][1][i][pi][3] if i == 0 else pc.chain(x[pi], g["angles1"][1, pi], g["zoom1"][1], g["noise1"][1, pi])[-1]
                assert np.abs(o - want).max() <= CHAIN_TOL
    # stages set to None are skipped, with their draws
    np.random.seed(3)
    before = np.random.get_state()[1].copy()
    x = tuple(tw["stage"][1][7][pi][0] for pi in range(3))
    out = dnn.augment_data(x, None, None, None)
    assert all(np.array_equal(a, b) for a, b in zip(out, x)) and np.array_equal(np.random.get_state()[1], before)


def test_status_codes_of_the_chain(rml):
    import torch
    from radar_ml_amd import _lib
    lib = _lib.load()
    ctx, st = _lib.context(), _lib.stream_ptr()
    p = torch.zeros((2, 8, 8), device="cuda")
    q = torch.full((2, 8, 8), 7.0, device="cuda")
    par = torch.zeros((2, 8), dtype=torch.float64, device="cuda")
    big = torch.zeros((1, 200, 200), device="cuda")
    out = torch.full((1, 200, 200), 7.0, device="cuda")
    call = lambda stages, src, stride, B, H, W, pr, dst: lib.rml_augment_chain(ctx, stages, _lib.ptr(src), stride, B, H, W, 127.5, 127.5, -1.0, 1.0, _lib.ptr(pr), _lib.ptr(dst), st)  # noqa: E731
    # a plane too large for the LDS: RML_ERR_UNSUPPORTED and nothing launched (480 KB with a spline stage, 160 KB without)
    assert call(7, big, 40000, 1, 200, 200, par, out) == -2 and b"LDS" in lib.rml_last_error()
    assert call(4, big, 40000, 1, 200, 200, par, out) == -2
    torch.cuda.synchronize()
    assert float(out.min()) == 7.0
    assert call(8, p, 64, 2, 8, 8, par, q) == -1 and b"stage" in lib.rml_last_error()
    assert call(7, p, 64, 2, 8, 8, None, q) == -1
    assert call(7, None, 64, 2, 8, 8, par, q) == -1
    assert call(7, p, 63, 2, 8, 8, par, q) == -1 and b"in_stride" in lib.rml_last_error()
    assert call(7, p, 64, 2, 0, 8, par, q) == -1
    assert call(7, None, 64, 0, 8, 8, None, None) == 0             # B == 0: a no-op
    torch.cuda.synchronize()
    assert float(q.min()) == 7.0
    assert call(0, p, 64, 2, 8, 8, None, q) == 0                   # the scaling alone needs no parameters
    torch.cuda.synchronize()
    assert float(q.max()) == -1.0


def test_fit_takes_device_tensors_bit_for_bit(rml):
    """Classifier.fit on 8 x 8 planes, 16 samples, 2 epochs, batch 8: CUDA tensors -- dense ones, and the strided planes of an (N, H, W, 3)
    tensor as dnn.train slices them -- give the history and the weights of the same arrays passed as NumPy"""
    import torch
    import dnn_train_common as S
    rng = np.random.default_rng(31)
    X, Xv = rng.uniform(-1, 1, (16, 8, 8, 3)).astype(np.float32), rng.uniform(-1, 1, (8, 8, 8, 3)).astype(np.float32)
    y, yv = rng.integers(0, 3, 16), rng.integers(0, 3, 8)
    results = {}
    for name in ("numpy", "dense", "strided"):
        m = S.make_model(8, 8, 3, 0, device="cuda").compile(seed=5, **S.ADAM)
        if name == "numpy":
            xs, vx = [X[..., k] for k in range(3)], [Xv[..., k] for k in range(3)]
        elif name == "dense":
            xs, vx = [torch.from_numpy(np.ascontiguousarray(X[..., k])).cuda() for k in range(3)], [torch.from_numpy(np.ascontiguousarray(Xv[..., k])).cuda() for k in range(3)]
        else:
            Xt, Xvt = torch.from_numpy(X).cuda(), torch.from_numpy(Xv).cuda()
            xs, vx = [Xt[..., k] for k in range(3)], [Xvt[..., k] for k in range(3)]
        hist = m.fit(xs, y, batch_size=8, epochs=2, validation_data=(vx, yv), class_weight={0: 2.0, 1: 1.0, 2: 1.5}).history
        loss, acc = m.train_on_batch([a[:5] for a in xs], y[:5])
        results[name] = (hist, [p.detach().cpu().numpy().copy() for p in m.parameters()], loss, acc)
        if name == "dense":            # a contiguous CUDA float32 tensor is kept as it is
            import radar_ml_amd.dnn as dnn
            assert dnn._planes(xs[0]).data_ptr() == xs[0].data_ptr()
    for name in ("dense", "strided"):
        assert results[name][0] == results["numpy"][0]
        assert results[name][2:] == results["numpy"][2:]
        for a, b in zip(results[name][1], results["numpy"][1]):
            np.testing.assert_array_equal(a, b)


def test_balance_gather_on_the_device(rml):
    """balance_classes on a CUDA tensor picks the rows it picks on the host"""
    import torch
    import radar_ml_amd.sgan as sgan
    rng = np.random.default_rng(2)
    data = rng.uniform(-1, 1, (9, 4, 4, 3)).astype(np.float32)
    labels, sup = np.array([0, 0, 1, 0, 2, 0, 1, 0, 1]), rng.random(9) < 0.5
    d0, l0, s0 = sgan.balance_classes(data, labels, sup, rng=np.random.default_rng(8))
    d1, l1, s1 = sgan.balance_classes(torch.from_numpy(data).cuda(), labels, sup, rng=np.random.default_rng(8))
    assert d1.is_cuda and d1.shape == (15, 4, 4, 3)
    np.testing.assert_array_equal(d1.cpu().numpy(), d0)
    np.testing.assert_array_equal(l1, l0)
    np.testing.assert_array_equal(s1, s0)


def test_sgan_train_takes_device_tensors(rml):
    """sgan.train for one epoch of two steps (32 x 32 planes, batch 8) with the data set as NumPy arrays and as the CUDA tensors
    preprocess_data(return_numpy=False) returns: the same models from the same seeds see the same bits on the device, so the two histories
    agree within the project's bound for the same rounds run twice (test_g_step_between_captured_heads: 2e-2; the half-precision
    convolution gradients are not bit-reproducible from run to run)."""
    import copy
    import torch
    import radar_ml_amd.sgan as sgan
    rng = np.random.default_rng(17)
    X, Xv = rng.uniform(-1, 1, (16, 32, 32, 3)).astype(np.float32), rng.uniform(-1, 1, (6, 32, 32, 3)).astype(np.float32)
    y, yv, sup = np.arange(16) % 3, np.arange(6) % 3, np.ones(16, bool)
    torch.manual_seed(5)
    d0 = sgan.Discriminator(((32, 32, 1),) * 3, 3).to("cuda").to(memory_format=torch.channels_last)
    d0.drop.p = 0.0
    g0 = sgan.Generator(latent_dim=16, channels=128, base=8, n_up=2).to("cuda").to(memory_format=torch.channels_last)
    hist = []
    for on_dev in (False, True):
        d, g = copy.deepcopy(d0), copy.deepcopy(g0)
        tr = sgan.DiscriminatorTrainer(d, amp_dtype="float16", ddp=False)
        gan = sgan.GanTrainer(g, tr)
        train_set = (torch.from_numpy(X).cuda(), y, sup) if on_dev else (X, y, sup)
        val_set = (torch.from_numpy(Xv).cuda(), yv) if on_dev else (Xv, yv)
        torch.manual_seed(6)
        h = sgan.train(g, tr, gan, train_set, val_set, 3, w_classes={0: 1.0, 1: 1.2, 2: 1.5}, latent_dim=16, n_epochs=1, n_batch=8, seed=3)
        hist.append(np.array(h))
    assert hist[0].shape == (2, 5) and np.isfinite(hist[0]).all() and np.isfinite(hist[1]).all()
    losses = [0, 2, 3, 4]                       # c, d on real, d on fake, g; column 1 is the c accuracy in steps of 1 / 4
    print("sgan.train NumPy against tensors: worst loss difference %.3g" % np.abs(hist[0] - hist[1])[:, losses].max())
    assert np.abs(hist[0] - hist[1])[:, losses].max() < 2e-2, hist
    assert hist[0][0, 1] == hist[1][0, 1]       # the first step's forward pass runs on the same weights and the same planes
