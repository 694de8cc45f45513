"""The engine's and the batched pipeline's host code on the CPU stand-in for the
device (tests/native/hipdouble/, tools/hipdouble_pipeline.sh): no GPU, no HIP
runtime in the link, AddressSanitizer + UBSan and ThreadSanitizer over every
schedule the stand-in offers.

  * the four scenarios of tests/native/pipeline_double_driver.c, one test per
    scenario and sanitizer, each over eager, lazy and seeds 1 .. 8: exit status
    0, no sanitizer report, no finding of the stand-in, "OK: 0 problems";
  * scenario b again with the stand-in showing one device, both lanes on it;
  * tests/native/hipdouble_selftest.cpp: every seeded mistake is caught with
    exactly its finding (or, for the deferred copy, its wrong bytes);
  * tests/hipdouble_forms.py: the stand-in's computing forms against the numpy
    references (oracle, gf256, pq_window).

Time limits: the slowest test here is scenario b on one device under
ThreadSanitizer (a store with two items past the 10 MiB window, ten schedules,
five at a time): 19 s on the machine the limits were taken on, so every test's
limit is 57 s, three times that -- the suite also runs on busier machines.  The build (once per
module) took 16 s and has 120 s."""
import concurrent.futures
import os
import platform
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(ROOT, "tools", "hipdouble_pipeline.sh")
SCHEDULES = ["eager", "lazy"] + [f"seed={n}" for n in range(1, 9)]
SLOWEST_S = 19
LIMIT_S = 3 * SLOWEST_S
REPORT = re.compile(r"(ERROR|WARNING): (Address|Thread|Leak|UndefinedBehavior)Sanitizer|runtime error:|SUMMARY: \w+Sanitizer")

pytestmark = pytest.mark.timeout(LIMIT_S, func_only=True)  # (the build has its own limit, in the fixture)


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """Both sanitizer builds and the unsanitized library, once per module."""
    out = tmp_path_factory.mktemp("hipdouble")
    env = dict(os.environ, BUILD_ONLY="1")
    r = subprocess.run(["bash", SCRIPT, str(out)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    return out


@pytest.fixture(scope="module")
def no_aslr():
    """ThreadSanitizer's fixed shadow layout wants no address-space randomisation
    (tools/tsan_pipeline.sh); where setarch may not switch it off, the binary runs as it is."""
    cmd = ["setarch", platform.machine(), "-R"]
    try:
        ok = subprocess.run(cmd + ["true"], capture_output=True, timeout=20).returncode == 0
    except OSError:
        ok = False
    return cmd if ok else []


def run(cmd, env=None, timeout=LIMIT_S):
    e = dict(os.environ)
    e.update({"ASAN_OPTIONS": "detect_leaks=0:halt_on_error=1",
              "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1",
              "TSAN_OPTIONS": "halt_on_error=1 second_deadlock_stack=1"})
    for k in ("HIPDOUBLE_LAZY_US", "HIPDOUBLE_LAUNCH_US", "HIPDOUBLE_TRACE", "HIPDOUBLE_DEVICES"):
        e.pop(k, None)
    e.update(env or {})
    return subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=e)


def test_binaries_do_not_link_the_hip_runtime(built):
    for san in ("address", "thread"):
        for prog in ("pipeline_double_driver", "hipdouble_selftest"):
            r = subprocess.run(["ldd", str(built / san / prog)], capture_output=True, text=True, timeout=30)
            assert r.returncode == 0, r.stderr
            assert "amdhip" not in r.stdout and "libhsa" not in r.stdout, r.stdout
    r = subprocess.run(["ldd", str(built / "plain" / "libbcp_double.so")], capture_output=True, text=True, timeout=30)
    assert r.returncode == 0 and "amdhip" not in r.stdout, r.stdout + r.stderr


def scenario_over_every_schedule(built, no_aslr, tmp_path, san, scenario, env=None):
    prog = str(built / san / "pipeline_double_driver")
    ldd = subprocess.run(["ldd", prog], capture_output=True, text=True, timeout=30)
    assert ldd.returncode == 0 and "amdhip" not in ldd.stdout, ldd.stdout + ldd.stderr
    prefix = no_aslr if san == "thread" else []

    def one(sched):
        store = tmp_path / sched.replace("=", "")
        return sched, run(prefix + [prog, scenario, str(store)], dict(env or {}, HIPDOUBLE_SCHEDULE=sched))

    with concurrent.futures.ThreadPoolExecutor(max_workers=5) as pool:
        results = list(pool.map(one, SCHEDULES))
    for sched, r in results:
        out = r.stdout + r.stderr
        where = f"scenario {scenario}, {san}, {sched}:\n{out[-6000:]}"
        assert r.returncode == 0, where
        assert not REPORT.search(out), where
        assert "FINDING" not in out and re.search(r"^hipdouble: 0 findings, [1-9]\d* operations$", r.stdout, re.M), where
        assert re.search(r"^OK: 0 problems$", r.stdout, re.M), where


@pytest.mark.parametrize("san", ["address", "thread"])
@pytest.mark.parametrize("scenario", ["a", "b", "c", "d"])
def test_scenario(built, no_aslr, tmp_path, san, scenario):
    scenario_over_every_schedule(built, no_aslr, tmp_path, san, scenario)


@pytest.mark.parametrize("san", ["address", "thread"])
def test_scenario_b_with_both_lanes_on_one_device(built, no_aslr, tmp_path, san):
    """The first faulting test ran on a machine with one GPU: its two lanes wrapped onto the same
    device, where up to two batches of a lane and three in all are on the device at once."""
    scenario_over_every_schedule(built, no_aslr, tmp_path, san, "b", {"HIPDOUBLE_DEVICES": "1"})


MISTAKES = {
    # case: (findings, what the one finding says)
    "src_past": (1, r"source \[0x[0-9a-f]+, \+4097\) runs 1 bytes past its device allocation"),
    "dst_past": (1, r"destination \[0x[0-9a-f]+, \+4097\) runs 1 bytes past its device allocation"),
    "cross_device": (1, r"source \[0x[0-9a-f]+, \+4096\) belongs to device 1, the stream to device 0"),
    "free_pending": (1, r"hipFree: \[0x[0-9a-f]+, \+4096\) is freed while xor_\w+.* still refers to"),
    "free_pending_uploaded": (1, r"hipFree: \[0x[0-9a-f]+, \+4096\) is freed while xor_\w+.* still refers to"),
    "pinned_rewrite": (0, None),
    "counter_bump": (1, r"the work-queue counter is (\d+) when the launch starts, its base (\d+)"),
}


@pytest.mark.parametrize("case", sorted(MISTAKES))
def test_stand_in_catches_seeded_mistake(built, case):
    want, text = MISTAKES[case]
    r = run([str(built / "address" / "hipdouble_selftest"), case])
    out = r.stdout + r.stderr
    assert r.returncode == 0 and not REPORT.search(out), out
    assert f"selftest {case}: findings={want} want={want} OK" in r.stdout, out
    found = [ln for ln in r.stderr.splitlines() if "FINDING" in ln]
    assert len(found) == want, out
    if text:
        m = re.search(text, found[0])
        assert m, found[0]
        if case == "counter_bump":
            assert int(m.group(1)) == int(m.group(2)) + 1, found[0]


def test_computing_forms_against_the_references(built):
    r = run([sys.executable, os.path.join(ROOT, "tests", "hipdouble_forms.py")],
            {"BCP_LIB": str(built / "plain" / "libbcp_double.so"), "HIPDOUBLE_SCHEDULE": "seed=5"})
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-6000:]
    m = re.search(r"^forms: (\d+) checks, 0 wrong$", r.stdout, re.M)
    assert m and int(m.group(1)) > 3000, out[-6000:]
    assert "FINDING" not in out, out[-6000:]
