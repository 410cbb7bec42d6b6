"""CNN training without a GPU: the case builder of tests/dnn_train_common.py meets its own conditions, the exported dropout mask
function, and the logic of Classifier.fit / dnn.train with the device function replaced by the float64 twin."""
import logging
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dnn_train_common as S  # noqa: E402
sys.path.pop(0)

from conftest import ROOT  # noqa: E402


@pytest.fixture(scope="module")
def D(rml):
    import radar_ml_amd.dnn as D
    return D


@pytest.mark.parametrize("shape", S.SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_case_builder_meets_its_conditions(D, shape):
    """float32 features bit-equal to float64, every trunk pre-activation >= 2^-13 from zero, ~47 % of the features live, dense
    pre-activations >= 1e-4 from zero, and no parameter tensor with a zero gradient"""
    import torch
    import torch.nn.functional as F
    H, W, B, C = shape
    c = S.case(*shape)
    m = S.make_model(H, W, C, c["seed"])
    params = list(m.parameters())
    xb = [torch.from_numpy(a[c["rows"].astype(np.int64)]) for a in c["xs"]]
    with torch.no_grad():
        f64 = S.twin_features([p.double() for p in params], xb, torch.float64)
        f32 = S.twin_features([p.float().contiguous() for p in params], xb, torch.float32)
        assert torch.equal(f32.double(), f64)
        for br in range(3):
            k1, b1, k2, b2 = (p.double() for p in params[4 * br:4 * br + 4])
            z1 = F.conv2d(F.pad(xb[br].double().unsqueeze(1), (0, 1, 0, 1)), k1, b1, stride=2)
            z2 = F.conv2d(F.pad(F.relu(z1), (0, 1, 0, 1)), k2, b2, stride=2)
            assert float(z1.abs().min()) >= S.TRUNK_MARGIN and float(z2.abs().min()) >= S.TRUNK_MARGIN
    live = float((f64 > 0).double().mean())
    print("%s: seed %d, %.1f %% of the features live" % (shape, c["seed"], 100 * live))
    assert 0.3 < live < 0.65
    for rate in S.RATES:
        t = c["t64"][rate]
        assert min(float(t["z1"].abs().min()), float(t["z2"].abs().min())) >= S.DENSE_MARGIN
        assert all(float(g.abs().max()) > 0 for g in t["grads"])
    assert len(c["rows"]) == B and len(c["y"]) > B and len(set(c["cw"])) == C


def test_dropout_mask_function(rml):
    a = S.keep_mask(5, 3, 0, 64, 0.5)
    assert np.array_equal(a, S.keep_mask(5, 3, 0, 64, 0.5))                                     # deterministic
    for other in (S.keep_mask(6, 3, 0, 64, 0.5), S.keep_mask(5, 4, 0, 64, 0.5), S.keep_mask(5, 3, 1, 64, 0.5)):
        assert not np.array_equal(a, other)                                                         # seed, step, layer
    for B in (1, 5, 37):
        assert np.array_equal(S.keep_mask(5, 3, 0, B, 0.5), a[:B])                                  # position b: the same at every B
    assert set(np.unique(a)) <= {0, 1} and S.keep_mask(5, 3, 0, 8, 0.0).all()
    # kept fraction: n draws at p = 1 - rate; six standard deviations
    for rate in (0.5, 0.25, 0.9):
        m = np.concatenate([S.keep_mask(11, t, l, 64, rate) for t in range(8) for l in range(2)]).reshape(-1)
        n, p = m.size, 1.0 - rate
        assert abs(m.mean() - p) <= 6.0 * np.sqrt(p * (1 - p) / n), (rate, m.mean())
    # neighbouring units / samples are not copies of each other
    assert 0.3 < (a[:, 1:] != a[:, :-1]).mean() < 0.7 and 0.3 < (a[1:] != a[:-1]).mean() < 0.7
    from radar_ml_amd import _lib
    assert _lib.load().rml_dnn_dropout_mask(0, 0, 0, 0, 4, 1.0, np.zeros(4, np.uint8).ctypes.data) == -1     # rate 1 drops everything


def test_symbols_and_supported(rml):
    from radar_ml_amd import _lib
    L = _lib.load()
    txt = open(os.path.join(ROOT, "include", "radarml.h")).read()
    for name in ("rml_dnn_train_supported", "rml_dnn_train_workspace_bytes", "rml_dnn_train_step", "rml_dnn_dropout_mask"):
        assert name in _lib.SIGNATURES and re.search(r"\b%s\s*\(" % name, txt) and hasattr(L, name)
    assert int(re.search(r"#define\s+RML_DNN_TRAIN_MAX_BATCH\s+(\d+)", txt).group(1)) == _lib.DNN_TRAIN_MAX_BATCH == 64
    assert L.rml_dnn_train_supported(80, 80, 3) and L.rml_dnn_train_supported(8, 8, 2) and L.rml_dnn_train_supported(12, 20, 5)
    for H, W in ((80, 82), (78, 80), (81, 80), (80, 6), (0, 80)):
        assert not L.rml_dnn_train_supported(H, W, 3)
        assert L.rml_dnn_train_workspace_bytes(64, H, W, 3) == 0
    assert not L.rml_dnn_train_supported(80, 80, 1) and not L.rml_dnn_train_supported(80, 80, 17)
    assert L.rml_dnn_train_workspace_bytes(64, 80, 80, 3) > 64 * 38400 * 4
    assert L.rml_dnn_train_workspace_bytes(65, 80, 80, 3) == 0 and L.rml_dnn_train_workspace_bytes(0, 80, 80, 3) == 0
    assert rml.define_classifier is __import__("radar_ml_amd.dnn", fromlist=["x"]).define_classifier


def test_workspace_covers_every_smaller_batch(rml):
    """rml_dnn_train_workspace_bytes(B) is enough for every batch of up to B samples (fit passes an epoch's partial last batch on the
    workspace of its batch_size): non-decreasing in B, at the reference's planes and at 40 x 40 (H/4 = 10 row splits to choose from)"""
    from radar_ml_amd import _lib
    L = _lib.load()
    for H, W, C in ((80, 80, 3), (40, 40, 3), (8, 8, 2), (12, 20, 5)):
        sizes = [int(L.rml_dnn_train_workspace_bytes(b, H, W, C)) for b in range(1, 65)]
        assert all(v > 0 for v in sizes)
        assert all(sizes[b] >= max(sizes[:b + 1]) for b in range(64)), (H, W, [b + 1 for b in range(1, 64) if sizes[b] < sizes[b - 1]])


def small_problem(n=40, nv=12, H=8, W=8, C=3, seed=0):
    rng = np.random.default_rng(77)
    xs = [a[..., None] for a in S.grid_planes(rng, n, H, W)]           # (N, H, W, 1), as Keras feeds them
    vx = S.grid_planes(rng, nv, H, W)
    y, vy = rng.integers(0, C, size=n), rng.integers(0, C, size=nv)
    return S.make_model(H, W, C, seed), xs, y, vx, vy


def test_fit_logic_with_the_twin(D, tmp_path):
    import torch
    m, xs, y, vx, vy = small_problem()
    m.compile(seed=3)
    twin = S.TwinTrainer(torch.float64)
    cw = {0: 5.48, 1: 1.26, 2: 1.0}
    with S.hooked(D, twin):
        h = m.fit(xs, y, batch_size=16, epochs=4, validation_data=(vx, vy), class_weight=cw)
    assert sorted(h.history) == ["accuracy", "loss", "val_accuracy", "val_loss"] and all(len(v) == 4 for v in h.history.values())
    assert h.epoch == [0, 1, 2, 3] and h.stopped_epoch is None and twin.steps == 12 == m._train_steps        # 16 + 16 + 8 per epoch
    # every epoch a fresh permutation of all rows, drawn from the seed
    rng = np.random.default_rng(3)
    for p in twin.perms:
        assert np.array_equal(p, rng.permutation(40)) and p.dtype == np.int32
    # epoch means with the partial last batch, class weights applied to the training loss alone: replay epoch 0 by hand
    m2, *_ = small_problem()
    params = [p.detach().double() for p in m2.parameters()]
    opt = torch.optim.Adam(params, lr=0.0002, betas=(0.5, 0.999), eps=1e-7)
    w = np.array([5.48, 1.26, 1.0], np.float32)
    planes = [a[..., 0] for a in xs]
    ls = co = 0
    for t, off in enumerate((0, 16, 32)):
        r = S.twin_step(params, planes, y, twin.perms[0][off:off + 16], w, 3, t, 0.5, torch.float64)
        for p, g in zip(params, r["grads"]):
            p.grad = g
        opt.step()
        ls, co = ls + r["loss_sum"], co + r["correct"]
    assert h.history["loss"][0] == pytest.approx(ls / 40, rel=1e-12) and h.history["accuracy"][0] == co / 40
    ev = S.twin_step(params, vx, vy, np.arange(12), None, 0, 0, 0.0, torch.float64, train=False)
    assert h.history["val_loss"][0] == pytest.approx(ev["loss_sum"] / 12, rel=1e-12) and h.history["val_accuracy"][0] == ev["correct"] / 12
    # the module holds the trained values when fit returns
    for p, q in zip(m.parameters(), twin.params):
        assert torch.equal(p.detach(), q.float())
    # no shuffle: the identity order
    m3, *_ = small_problem()
    t3 = S.TwinTrainer(torch.float64)
    with S.hooked(D, t3):
        m3.fit(xs, y, batch_size=64, epochs=1, shuffle=False)
    assert np.array_equal(t3.perms[0], np.arange(40)) and t3.steps == 1
    with pytest.raises(ValueError):
        m3.fit(xs, y, patience=2)                      # val_loss needs validation data
    with pytest.raises(ValueError):
        m3.fit(xs, np.where(y == 0, 3, y))             # a label outside [0, C)


def test_early_stopping_and_checkpoint(D, tmp_path):
    """a scripted val_loss: best at epoch 2; patience 3 stops after epoch 5; the file holds epoch 2's weights, the model epoch 5's"""
    import torch
    m, xs, y, vx, vy = small_problem()
    script = [0.9, 0.8, 0.5, 0.6, 0.5, 0.7, 0.1, 0.1]
    seen = []

    def fake(model, job, perm):
        ep = len(seen)
        seen.append(ep)
        with torch.no_grad():
            model.fc3.bias.fill_(float(ep))
        return 1.0 * len(job.y), len(job.y) // 2, script[ep] * len(job.val_y), len(job.val_y)

    fp = str(tmp_path / "best.pt")
    with S.hooked(D, fake):
        h = m.fit(xs, y, epochs=8, validation_data=(vx, vy), patience=3, checkpoint=fp)
    assert seen == [0, 1, 2, 3, 4, 5] and h.stopped_epoch == 5                 # 0.5 at epoch 4 is not BELOW the best
    assert h.history["val_loss"] == pytest.approx(script[:6]) and h.history["loss"] == [1.0] * 6 and h.history["accuracy"] == [0.5] * 6
    assert float(torch.load(fp)["fc3.bias"][0]) == 2.0 and float(m.fc3.bias.detach()[0]) == 5.0
    assert sorted(torch.load(fp)) == sorted(m.state_dict())


def test_train_emits_the_reference_log_lines(D, tmp_path, caplog):
    import torch
    m, xs, y, vx, vy = small_problem()
    X = np.concatenate(xs, axis=-1)                                             # (N, H, W, 3)
    Xv = np.stack(vx, axis=-1)
    with S.hooked(D, S.TwinTrainer(torch.float64)), caplog.at_level(logging.INFO):
        h = D.train(m, X, y, Xv, vy, {0: 5.48, 1: 1.26, 2: 1.0}, str(tmp_path), epochs=3)
    lines = [r.getMessage() for r in caplog.records]
    i = int(np.argmin(h.history["val_loss"]))
    assert lines[0] == "Training model."
    assert "Best loss: %.4f, Best acc: %.2f%%" % (h.history["loss"][i], 100 * h.history["accuracy"][i]) in lines
    assert "Best val loss: %.4f, Best val acc: %.2f%%" % (h.history["val_loss"][i], 100 * h.history["val_accuracy"][i]) in lines
    assert lines[-1] == "Saved best model to %s" % tmp_path
    assert re.fullmatch(r"Best loss: \d+\.\d{4}, Best acc: \d+\.\d\d%", lines[-3])
    assert sorted(torch.load(str(tmp_path / "c_model.pt"))) == sorted(m.state_dict())


def test_fit_has_no_cpu_path(D):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    m, xs, y, vx, vy = small_problem()
    from radar_ml_amd import RadarMLError
    with pytest.raises(RadarMLError):
        m.fit(xs, y, epochs=1)
