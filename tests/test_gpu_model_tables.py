"""GPU: a whole model build, table by table, through oslam_model_tables_tap.

Every cloud of tests/model_inputs.py is built on the device and its tables are held to the restatement
(tests/model_ref.py: hold): the slot tables (key sets, lengths, probe reachability, the scan, the marker flag, the
growth of cap), the entries (per bucket the multiset of (word, mi), per segment the spread's dealing, every padding
word), the second order (per segment the stable sort by P of the device's own segment and its directory, per bucket the
multiset of (word, uv bits)), the union table, the weights, the key numbers, reach, the key map and uinfo with its
stride padding.  Integers and floats' bit patterns only: no tolerance.  Then the parameter variants, a saved and loaded
model, and a database group of two unequal models.  tests/test_model_tables_host.py proves on the CPU that every cloud
reaches its edge and that hold() refuses tables that are wrong in one place."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import model_inputs as I  # noqa: E402
import model_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


def _built(ppf, p, nr, d, **params):
    return ppf.Model(p, nr, d_dist=d, params=ppf.default_params(**params) if params else None)


@pytest.mark.parametrize("name", sorted(I.CLOUDS))
def test_tables_hold(ppf, oracle, name):
    p, nr, d, m, u = I.reference(name, oracle, ppf)
    model = _built(ppf, p, nr, d)
    T = model.tables()
    model.close()
    R.hold(T, m, u)


@pytest.mark.parametrize("name", ["small", "markers", "points_1023"])
@pytest.mark.parametrize("variant", ["fast", "no_spread", "slot_order"])
def test_parameter_variants_hold(ppf, oracle, name, variant):
    p, nr, d, m, u = I.reference(name, oracle, ppf)
    params, kw = {"fast": (dict(vote_mode=ppf.VOTE_FAST), dict(fast=True)),
                  "no_spread": (dict(no_bucket_spread=1), dict(spread=False)),
                  "slot_order": (dict(vote_order=1), dict(vote_order=1))}[variant]
    model = _built(ppf, p, nr, d, **params)
    T = model.tables()
    model.close()
    assert T["has_pw"] == (variant != "fast")
    R.hold(T, m, u, **kw)


@pytest.mark.parametrize("name", ["small", "markers"])
def test_saved_and_loaded_model_is_the_same(ppf, oracle, tmp_path, name):
    p, nr, d, m, u = I.reference(name, oracle, ppf)
    model = _built(ppf, p, nr, d)
    A = model.tables()
    path = str(tmp_path / "model.bin")
    model.save(path)
    model.close()
    loaded = ppf.Model.load(path)
    Bt = loaded.tables()
    loaded.close()
    R.hold(Bt, m, u)
    for k in ("slots", "ukeys", "reach", "e4", "mi", "uids", "weights", "kmap", "uinfo"):
        assert np.array_equal(A[k], Bt[k]), k
    flat = A["slots"].reshape(-1, 4)
    entry, directory = R.second_order_places(flat[:, 1], np.where(flat[:, 0] != 0, flat[:, 2], 0))
    assert len(entry) == len(m.key)
    assert np.array_equal(A["pw"][entry], Bt["pw"][entry]) and np.array_equal(A["pdir"][directory], Bt["pdir"][directory])
    assert np.array_equal(A["puv"].view(np.uint32)[entry], Bt["puv"].view(np.uint32)[entry])


def test_group_members_share_the_union_and_keep_their_buckets(ppf, oracle):
    pa, na, d, ma, ua = I.reference("small", oracle, ppf)
    pb, nb, _, mb, ub = I.reference("small_other", oracle, ppf)
    union = R.Union([ma, mb], d)
    assert union.n_ids > max(ua.n_ids, ub.n_ids)
    models = [_built(ppf, pa, na, d), _built(ppf, pb, nb, d)]
    db = ppf.Database(models)
    assert db.n_groups == 1
    Ta, Tb = models[0].tables(), models[1].tables()
    db.close()
    for x in models:
        x.close()
    for k in ("ukeys", "uids", "weights", "reach", "kmap"):                  # one table for both
        assert np.array_equal(Ta[k], Tb[k]), k
    R.hold(Ta, ma, union)
    R.hold(Tb, mb, union)
    assert Ta["uinfo"].shape != Tb["uinfo"].shape or not np.array_equal(Ta["uinfo"], Tb["uinfo"])
