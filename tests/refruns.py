"""The reference binary's side of the side-by-side tests, recorded: tests/golden/reference_runs.json.xz holds what
oracle/_ref/parsnp_core_ref returned for every case, so that the tests need nothing outside the repository.  A result is
keyed by what the binary reads (the name and bytes of every input file, the ini settings) and by the test helper that
summarised its run; tests/golden/muscle_runs.json.xz holds what oracle/_ref/muscle_ref (libMUSCLE) aligned (tests/gapgen.py).
A case with no record runs the binary where it has been built, and fails where it has not.  tests/golden/make_reference_runs.py
records the results: with PARSNP_REF_RECORD=<dir> every test writes the reference's result of its case into <dir> and skips
the product's side."""
import hashlib
import json
import lzma
import os

import pytest

import oracles

REFBIN = os.path.join(oracles.REFDIR, "parsnp_core_ref")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_runs.json.xz")
_golden = {}


def normal(result):
    """a run's result as it reads back from JSON (tuples become lists): compare the product's side in this form"""
    return json.loads(json.dumps(result))


def case_key(run, rp, qs, *rest):
    h = hashlib.sha256()
    h.update(("%s.%s\n" % (run.__module__, run.__name__)).encode())
    for p in [rp] + list(qs):
        data = open(p, "rb").read()
        h.update(("%s %d\n" % (os.path.basename(p), len(data))).encode())
        h.update(data)
    h.update(json.dumps(rest, sort_keys=True).encode())
    return h.hexdigest()


def reference(run, rp, qs, out, *rest):
    """run(REFBIN, rp, qs, out, *rest), normal(), from the record of the case"""
    return recorded(GOLDEN, case_key(run, rp, qs, *rest), REFBIN, lambda: run(REFBIN, rp, qs, out, *rest))


def recorded(golden, key, binary, compute):
    """normal(compute()) -- what the reference program `binary` gives -- from the record `key` of the file `golden`;
    without a record, computed where the program has been built; with PARSNP_REF_RECORD, computed, recorded and the test skipped"""
    record = os.environ.get("PARSNP_REF_RECORD")
    if record:
        result = normal(compute())
        os.makedirs(os.path.join(record, os.path.basename(golden)), exist_ok=True)
        with open(os.path.join(record, os.path.basename(golden), key + ".json"), "w") as f:
            json.dump(result, f)
        pytest.skip("reference result recorded")
    if golden not in _golden:
        _golden[golden] = json.load(lzma.open(golden, "rt")) if os.path.exists(golden) else {}
    if key in _golden[golden]:
        return _golden[golden][key]
    if not os.path.exists(binary):
        pytest.fail("no recorded result of %s for this case in %s (tests/golden/make_reference_runs.py)" % (os.path.basename(binary), os.path.relpath(golden)))
    return normal(compute())
