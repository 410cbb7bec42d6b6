"""Makes tests/golden/train_flow.npz from the reference's own functions (run once, where the reference is at hand):

    python tests/golden/make_golden_train_flow.py <directory of the reference's train.py>

It imports the reference's ``train.py`` and records
  * ``balance_classes`` on three label sets (balanced, unbalanced in three classes, one class of three absent);
  * the batches the augment loop of ``sgd_fit`` (train.py:425-438) hands to ``partial_fit`` for a 40-sample set with seeded
    ``np.random``: per batch the labels before balancing and which positions of the batch the balanced set holds, in its
    order (``balance_classes`` run on the positions in place of the feature rows).  (The noisy tuples are drawn from an unseeded generator: their values differ from run to run, their
    places do not.)
Nothing of the reference's source is copied: only inputs and recorded outputs are stored."""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FLOW_SEED = 7
FLOW_SHAPES = ((4, 5), (6, 5), (4, 6))
FLOW_BATCH = 16


def flow_set():
    """40 samples of small planes in three unbalanced classes (18 / 14 / 8)."""
    rng = np.random.RandomState(3)
    y = np.array([0] * 18 + [1] * 14 + [2] * 8)
    rng.shuffle(y)
    x = [tuple(rng.rand(*s).astype(np.float32) for s in FLOW_SHAPES) for _ in y]
    return x, y


def label_sets():
    rng = np.random.RandomState(4)
    sets = {"balanced": np.array([0, 1, 2] * 5), "unbalanced": np.array([2] * 9 + [0] * 4 + [1] * 6), "absent": np.array([0] * 7 + [2] * 3)}
    out = {}
    for name, lab in sets.items():
        rng.shuffle(lab)
        out[name] = (lab, rng.rand(len(lab), 6).astype(np.float32))
    return out


def main(ref):
    sys.path.insert(0, ref)
    stub = types.ModuleType("WalabotAPI")             # the radar's driver: imported by common.py, not used here
    stub.PROF_SENSOR = 0
    sys.modules["WalabotAPI"] = stub
    os.environ.setdefault("MPLBACKEND", "Agg")
    import common
    import train
    out = {}
    for name, (lab, data) in label_sets().items():
        lb, db = train.balance_classes(lab, data)
        out["bal_%s_labels" % name], out["bal_%s_data" % name] = lab, data
        out["bal_%s_out_labels" % name], out["bal_%s_out_data" % name] = np.asarray(lb), np.asarray(db)
    x, y = flow_set()
    np.random.seed(FLOW_SEED)
    gen = train.DataGenerator(rotation_range=5.0, zoom_range=0.2, noise_sd=0.1, balance=True)
    batch = 0
    for X_batch, y_batch in gen.flow(x, y, batch_size=FLOW_BATCH):
        # balancing draws by position only: the positions stand in for the feature rows the loop would pass
        yb, Xb = train.balance_classes(y_batch, np.arange(len(y_batch)).reshape(-1, 1))
        idx = np.asarray(Xb)[:, 0]
        assert len(X_batch) == len(y_batch) and (np.asarray(y_batch)[idx] == yb).all()
        out["flow_%d_labels" % batch], out["flow_%d_index" % batch] = np.asarray(y_batch), idx
        out["flow_%d_balanced" % batch] = np.asarray(yb)
        batch += 1
        if batch >= len(x) / FLOW_BATCH:
            break
    out["flow_batches"] = np.array(batch)
    np.savez_compressed(os.path.join(HERE, "train_flow.npz"), **out)
    print("wrote train_flow.npz: %d arrays, %d batches" % (len(out), batch))


if __name__ == "__main__":
    main(sys.argv[1])
