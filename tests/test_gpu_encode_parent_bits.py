"""The encoding host path (EncodeBasis, encode_tables, the shared kernel prologue) changes no arithmetic: every output of the device-side
encoders equals, byte for byte, what the build of the commit before it produced on the same GPU model
(tests/golden/encode_host_path/parent.npz, recorded by tests/golden/make_encode_parent.py, which also generates the inputs here;
the commit and the toolchain are in the file's meta_* entries).  All four kinds of basis through the four doors - encode_values for a
training and a test set, encode_dataset + get_encoded in the basis' own type and through the cast - with the returned norms and
out-of-bounds lists."""
import importlib.util
import os

import numpy as np
import pytest

import mpstime_jl_amd as mt

pytestmark = pytest.mark.gpu

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDEN = os.path.join(GOLDEN_DIR, "encode_host_path", "parent.npz")       # (a directory of its own: tests/golden/*.npz are sweep fixtures)


def _recorder():
    spec = importlib.util.spec_from_file_location("make_encode_parent", os.path.join(GOLDEN_DIR, "make_encode_parent.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def recorded():
    """(recorder module, the current build's outputs - computed once -, the fixture)"""
    rec = _recorder()
    return rec, rec.outputs(mt), np.load(GOLDEN)


def test_every_recorded_output_is_produced(recorded):
    rec, got, gold = recorded
    want = {k[len("sha/"):] for k in gold.files if k.startswith("sha/")}
    assert set(got) == want and len(want) >= 4 * len(rec.ARRAYS)
    assert {k[len("arr/"):] for k in gold.files if k.startswith("arr/")} == set(rec.ARRAYS)


def test_bits_equal_the_parent_build(recorded):
    rec, got, gold = recorded
    for case in rec.ARRAYS:                                    # the arrays first: a mismatch is located before any digest is compared
        a, ref = got[f"{case}/values_train/phi"], gold["arr/" + case]
        assert a.shape == ref.shape and a.dtype == ref.dtype, case
        bad = np.argwhere(a != ref)
        assert bad.size == 0, (case, len(bad), bad[0].tolist(), float(np.abs(a - ref).max()))
    differ = [k for k, a in got.items() if rec.digest(a) != str(gold["sha/" + k])]
    assert not differ, differ
