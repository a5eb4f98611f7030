"""State that lives from step to step of one CoreRun: the MUM and LCB lists written on first use after a chain on the device, the
vectors a step borrows from AlignerMemory, the capacities an engine call takes from the same call of the step before.  One
process, four steps that mix the report with and without the LCBs' reference intervals, the writer after steps 2 and 4: every
step must say the same, both XMFAs must be the reference's bytes (tests/golden/e2e.json).

Routes of the parent commit on these inputs under PARSNP_PARALLEL_MIN=8 PARSNP_FREE_MIN=2 PM_DIRTY_MIN=8 (emulation, recorded from
a run of the parent):  pop6x200k resident=1 device_chain=1; rearr6x300k resident=1 device_chain=1; popinv12x400k resident=1
device_chain=1.
"""
import json
import os
import subprocess
import sys

import pytest

import test_host_logic
from parsnp_amd import driver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(PARSNP_PARALLEL_MIN="8", PARSNP_FREE_MIN="2", PM_DIRTY_MIN="8")
# (input, resident, device_chain) as the parent commit takes them
ROUTES = {"pop6x200k": (1, 1), "rearr6x300k": (1, 1), "popinv12x400k": (1, 1)}

CHILD = r"""
import sys, json, hashlib, os
sys.path.insert(0, %(root)r)
from parsnp_amd.core_api import CoreRun
r = CoreRun(%(ini)r, lib_path=%(lib)r)
out = {"steps": [], "md5": []}
for k, intervals in enumerate((True, False, True, False)):
    s = r.step(intervals=intervals)
    out["steps"].append({"mums": s["mums"], "lcbs": s["lcbs"], "core_bp": s["core_bp"], "anchors": s["anchors"], "resident": s["resident"],
                         "device_chain": s["device_chain"], "resident_retry": s["resident_retry"], "tail_repeats": s["engine_ms"].get("tail_repeats", 0),
                         "intervals": s["lcb_ref_intervals"]})
    if k in (1, 3):
        assert r.write() == 0
        out["md5"].append(hashlib.md5(open(os.path.join(%(out)r, "parsnpAligner.xmfa"), "rb").read()).hexdigest())
r.close()
print("RESULT " + json.dumps(out))
"""


def four_steps(lib, name, base, extra_env=None):
    rp, qs, kw = test_host_logic.harsh_inputs(name, base)
    out = os.path.join(base, "out")
    os.makedirs(out)
    ini = os.path.join(out, "parsnpAligner.ini")
    open(ini, "w").write(driver.ini_text(rp, qs, out, threads=2, **kw))
    env = dict(os.environ, **ENV)
    env.update(extra_env or {})
    p = subprocess.run([sys.executable, "-c", CHILD % dict(root=ROOT, ini=ini, lib=lib, out=out)], capture_output=True, text=True, env=env, cwd=out)
    assert p.returncode == 0, p.stdout[-1000:] + p.stderr[-3000:]
    line = [x for x in p.stdout.splitlines() if x.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def check(res, name):
    resident, device_chain = ROUTES[name]
    steps = res["steps"]
    assert len(steps) == 4
    for s in steps:
        assert s["resident"] == resident and s["device_chain"] == device_chain and s["resident_retry"] == 0, s
        for key in ("mums", "lcbs", "core_bp", "anchors"):
            assert s[key] == steps[0][key], (key, [t[key] for t in steps])
    assert steps[0]["mums"] > 0 and steps[0]["lcbs"] > 0 and steps[0]["core_bp"] > 0
    assert steps[0]["intervals"] and steps[0]["intervals"] == steps[2]["intervals"]
    assert steps[1]["intervals"] == [] and steps[3]["intervals"] == []
    assert sum(b - a + 1 for a, b in steps[0]["intervals"]) == steps[0]["core_bp"]
    want = test_host_logic.E2E[name]["xmfa_md5"]
    assert res["md5"] == [want, want]


def emu_core_lib(emu):
    return os.path.join(os.path.dirname(emu[0]), "libparsnp_core_emu.so")


@pytest.mark.parametrize("name", ["pop6x200k", "rearr6x300k", "popinv12x400k"])
def test_four_steps_one_run(emu, tmp_path, name):
    check(four_steps(emu_core_lib(emu), name, str(tmp_path)), name)


def test_capacities_too_small(emu, tmp_path):
    """hint_shrink divides what a call carries over from the step before: every later step repeats the parts that needed it, and
    nothing else changes"""
    res = four_steps(emu_core_lib(emu), "pop6x200k", str(tmp_path), {"PM_HINT_SHRINK": "64"})
    check(res, "pop6x200k")
    assert res["steps"][0]["tail_repeats"] == 0          # (the first step has nothing to carry over)
    assert all(s["tail_repeats"] > 0 for s in res["steps"][1:]), [s["tail_repeats"] for s in res["steps"]]


@pytest.mark.gpu
def test_four_steps_one_run_on_the_device(tmp_path):
    """the first case on the HIP library (the test hooks that put a small set on the resident route are compiled into the emulation's host
    code only: the engine's threshold is set through bench-style tuning of the session instead)"""
    from parsnp_amd.core_api import CORE_LIB
    name = "pop6x200k"
    rp, qs, kw = test_host_logic.harsh_inputs(name, str(tmp_path))
    out = str(tmp_path / "out")
    os.makedirs(out)
    ini = os.path.join(out, "parsnpAligner.ini")
    open(ini, "w").write(driver.ini_text(rp, qs, out, threads=2, **kw))
    child = CHILD.replace("r = CoreRun(%(ini)r, lib_path=%(lib)r)\n",
                          "r = CoreRun(%(ini)r, lib_path=%(lib)r)\n"
                          "import ctypes as C\n"
                          "r.L.pc_tune.argtypes = [C.c_void_p, C.c_char_p, C.c_longlong]\n"
                          "assert r.L.pc_tune(r.h, b'dirty_min', 8) == 0\n")
    p = subprocess.run([sys.executable, "-c", child % dict(root=ROOT, ini=ini, lib=CORE_LIB, out=out)], capture_output=True, text=True, cwd=out)
    assert p.returncode == 0, p.stdout[-1000:] + p.stderr[-3000:]
    res = json.loads([x for x in p.stdout.splitlines() if x.startswith("RESULT ")][-1][len("RESULT "):])
    check(res, name)
