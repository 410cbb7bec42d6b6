"""Writes tests/golden/prep_golden.npz: what the reference's ``augment_data`` / ``preprocess_data`` / ``balance_classes`` (dnn.py, sgan.py)
make of a nine-sample data set -- six samples at the Walabot projection shapes 22x176 / 31x176 / 22x31 and three at 5x7 / 7x5 / 5x5, the
smallest planes where crop, paste, trim and the mirror indices can go wrong; float32 planes holding sparse integers 0..255, one sample
scaled off the integer grid; classes of 5 / 3 / 1 samples with a supervised mask.

Like make_golden.py it runs only where the reference tree is present and imports it (dnn.py / sgan.py with stub ``tensorflow`` and
``WalabotAPI`` modules); nothing of the reference's source is copied.  Recorded: every draw (both random sources are wrapped while the reference runs),
the planes after rotate, after zoom and after noise (``augment_data`` called with the later stages set to None) for two settings -- the
defaults (1.0, 0.3, 1.0) and (15.0, 0.3, 0.05), where corners leave the plane and the noise does not saturate it -- and the results of
both modules' ``preprocess_data`` with and without ``augment`` at ``train_split`` 0.8.  Draws, orders, labels, masks, weights and the
stage planes of one Walabot sample and the small ones are stored in full; the large arrays (9 samples x 128 x 128 x 3 per run) as SHA-256 digests of dtype, shape
and bytes (tests/prep_common.digest), which is all a bit-for-bit comparison needs.  ``python tests/golden/make_golden_prep.py``."""
import hashlib
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
SETTINGS = ((1.0, 0.3, 1.0), (15.0, 0.3, 0.05))
SHAPES_W = ((22, 176), (31, 176), (22, 31))
SHAPES_S = ((5, 7), (7, 5), (5, 5))
LABELS = ["person", "dog", "person", "cat", "person", "dog", "person", "dog", "person"]
FULL = (0, 6, 7, 8)         # samples whose stage planes are stored in full: one Walabot sample and the small ones
SUP = [True, True, False, True, True, False, True, True, False]


def digest(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha256(str((a.dtype.str, a.shape)).encode() + a.tobytes()).hexdigest()


def import_reference():
    for stub in ("tensorflow", "WalabotAPI"):           # imported at module level, used by neither function recorded here
        sys.modules.setdefault(stub, types.ModuleType(stub))
    sys.modules["WalabotAPI"].PROF_SENSOR = 0
    os.environ.setdefault("MPLBACKEND", "Agg")
    sys.path.insert(0, REF)
    import dnn
    import sgan
    return dnn, sgan


class Recorder:
    """wraps np.random.uniform and a module's ``rng`` while the reference runs"""

    def __init__(self, mod, np_seed):
        self.mod, self.uniform, self.normal, self.shuffles = mod, [], [], []
        np.random.seed(np_seed)
        self.gen = np.random.default_rng(1234)

    def __enter__(self):
        self._uniform, self._rng = np.random.uniform, self.mod.rng
        rec = self

        def uniform(*a, **k):
            v = rec._uniform(*a, **k)
            rec.uniform.append(v)
            return v

        class Rng:
            def normal(self, *a, **k):
                v = rec.gen.normal(*a, **k)
                rec.normal.append(v)
                return v

            def shuffle(self, x):
                rec.gen.shuffle(x)
                rec.shuffles.append(np.array(x))

        np.random.uniform, self.mod.rng = uniform, Rng()
        return self

    def __exit__(self, *exc):
        np.random.uniform, self.mod.rng = self._uniform, self._rng
        return False


def make_inputs():
    rng = np.random.default_rng(77)

    def planes(n, shape):
        v = rng.integers(1, 256, (n,) + shape).astype(np.float32)
        v[rng.random((n,) + shape) < 0.4] = 0.0            # sparse, as radar projections are
        return v
    w = [planes(6, s) for s in SHAPES_W]
    s = [planes(3, s) for s in SHAPES_S]
    for p in w:
        p[1] = (p[1] * np.float32(0.9371)).astype(np.float32)       # one sample off the integer grid
    return w, s


def staged(ref, data, setting, np_seed):
    """per sample: augment_data with one stage at a time, each on the previous one's result -- the draws come in the order of the full call"""
    rot, zr, sd = setting
    with Recorder(ref, np_seed) as rec:
        out = []
        for smp in data:
            x = tuple((p - 255.0 / 2.) / (255.0 / 2.) for p in smp)
            r = ref.augment_data(tuple(p.copy() for p in x), rot, None, None)
            z = ref.augment_data(tuple(p.copy() for p in r), None, zr, None)
            nz = ref.augment_data(tuple(p.copy() for p in z), None, None, sd)
            out.append((r, z, nz))
    n = len(data)
    u = np.array(rec.uniform).reshape(n, 4)
    return out, u[:, :3], u[:, 3], np.array(rec.normal).reshape(n, 3)


def conditions(runs):
    zooms = np.concatenate([r[2] for r in runs])
    final = np.concatenate([p.ravel() for smp in runs[1][0] for p in smp[2]])
    inside = np.mean((final > -1.0) & (final < 1.0))
    return inside >= 0.5 and (zooms < 1.0).any() and (zooms > 1.0).any(), inside


def main():
    from PIL import Image
    dnn, sgan = import_reference()
    w, s = make_inputs()
    data = [tuple(p[i] for p in w) for i in range(6)] + [tuple(p[i] for p in s) for i in range(3)]
    out = {"labels": np.array(LABELS), "sup": np.array(SUP)}
    for k in range(3):
        out["w%d" % k], out["s%d" % k] = w[k], s[k]

    # seeds for which the reference meets the conditions (one np.random seed per setting; the module generators are default_rng(1234))
    seeds = None
    for s0 in range(100, 140):
        runs = [staged(dnn, data, SETTINGS[0], s0), staged(dnn, data, SETTINGS[1], s0 + 1000)]
        ok, inside = conditions(runs)
        if ok:
            seeds = (s0, s0 + 1000)
            break
    assert seeds is not None, "no seed meets the conditions"
    print("np.random seeds", seeds, "setting 1: %.1f %% of the final pixels strictly inside (-1, 1)" % (100 * inside))
    for k, (planes, angles, zoom, noise) in enumerate(runs):
        assert (zoom < 1.0).any() and (zoom > 1.0).any()
        out["np_seed%d" % k] = np.int64(seeds[k])
        out["setting%d" % k] = np.array(SETTINGS[k])
        out["angles%d" % k], out["zoom%d" % k], out["noise%d" % k] = angles, zoom, noise
        out["stage_digest%d" % k] = np.array([[[digest(planes[i][st][pi]) for st in range(3)] for pi in range(3)] for i in range(9)])
        for i in FULL:
            for pi in range(3):
                out["stage%d_%d_%d" % (k, i, pi)] = np.stack([planes[i][st][pi] for st in range(3)])
        # sgan.py's augment_data is the same function: same draws, same planes
        again = staged(sgan, data, SETTINGS[k], seeds[k])
        assert all(np.array_equal(a, b) for sa, sb in zip(planes, again[0]) for ta, tb in zip(sa, sb) for a, b in zip(ta, tb))
    final1 = runs[1][0]
    out["resized_digest1"] = np.array([[digest(np.asarray(Image.fromarray(final1[i][2][pi]).resize((80, 80), resample=Image.BICUBIC)))
                                        for pi in range(3)] for i in range(9)])

    for name, ref in (("dnn", dnn), ("sgan", sgan)):
        for aug in (0, 1):
            args = types.SimpleNamespace(augment=bool(aug), train_split=0.8)
            with Recorder(ref, seeds[0]) as rec:
                if name == "dnn":
                    X_train, y_train, X_val, y_val, n_classes, w_classes = ref.preprocess_data(args, data, LABELS)
                else:
                    (X_bal, y_bal, sup_bal), (X_val, y_val), n_classes, w_classes = ref.preprocess_data(args, data, LABELS, SUP)
            key = "%s_%d_" % (name, aug)
            if aug:         # the full call made the staged run's draws
                assert np.array_equal(np.array(rec.uniform).reshape(9, 4)[:, :3], out["angles0"]) and np.array_equal(np.array(rec.normal).reshape(9, 3), out["noise0"])
            out[key + "order"] = rec.shuffles[0]
            if name == "sgan":
                # the training part before balancing is not returned: the balanced set, its labels and mask and the balance's own
                # shuffle pin the resampled rows
                assert len(rec.shuffles) == 2 and len(y_bal) == len(rec.shuffles[1]) and X_bal.shape[1:] == (128, 128, 3)
                out[key + "X_bal"], out[key + "y_bal"], out[key + "sup_bal"] = np.array(digest(X_bal)), y_bal, sup_bal
                out[key + "bal_shuffle"] = rec.shuffles[1]
            else:
                out[key + "X_train"], out[key + "y_train"] = np.array(digest(X_train)), y_train
                assert X_train.shape == (7, 80, 80, 3) and X_train.dtype == np.float32
            out[key + "X_val"], out[key + "y_val"] = np.array(digest(X_val)), y_val
            out[key + "n_classes"] = np.int64(n_classes)
            ks = sorted(w_classes)
            out[key + "w_keys"], out[key + "w_vals"] = np.array(ks), np.array([w_classes[c] for c in ks])
    path = os.path.join(HERE, "prep_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
