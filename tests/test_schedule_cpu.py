"""Where the parts of a batch run, without a GPU: the decision of csrc/schedule.h built with a host compiler
(tests/schedule_host.cpp) and pinned row by row against the table in that header.  The expected streams here are written
out by hand from the table, not computed: a change of schedule has to change this file too.

M = compute, F / F2 = flat / flat2, U = upload, C = copy, L / L2 = latest / latest2."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M, F, F2, C, U, L, L2 = "compute", "flat", "flat2", "copy", "upload", "latest", "latest2"

# the default job: no switch set, untimed, the host half of the fold, the wide chain, 64 4:2:0 frames a launch, an even slot
DEFAULT = dict(one_stream=0, no_defer=0, side2=0, w_aside=0, f_serial=0, d2h_sync=0, timed=0, device_latest=0, wide=1, batch=64, slot=2,
               nplanes=3, last_back=1)
FIELDS = ("table", "finder", "accum", "rest", "latest", "d2h", "back_now", "after", "host_waits")


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path_factory.mktemp("schedule") / "schedule_host"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-o", str(exe), os.path.join(ROOT, "tests", "schedule_host.cpp")])

    def ask(**changes):
        assert not set(changes) - set(DEFAULT), changes
        job = dict(DEFAULT, **changes)
        out = subprocess.run([str(exe)] + [str(job[k]) for k in DEFAULT], capture_output=True, text=True, check=True).stdout.split()
        assert len(out) == len(FIELDS), out
        s = dict(zip(FIELDS, out))
        s["back_now"], s["after"] = bool(int(s["back_now"])), int(s["after"])
        if not job["device_latest"]:
            del s["latest"]  # (nothing runs on it: the table gives it no stream)
        return s

    return ask


def test_the_default_job(plan):
    """The table on the upload stream, the finder chain on the side stream, the accumulation and its tail on the main stream,
    the records by the copy stream; the back half deferred, no wait for a batch before, none on the host."""
    assert plan() == dict(table=U, finder=F, accum=M, rest=M, d2h=C, back_now=False, after=-1, host_waits="none")
    assert plan(slot=3) == plan()  # (the slot's parity alone moves nothing)
    assert plan(batch=32) == plan() and plan(last_back=-1) == plan()


def test_the_window_from_64_frames_a_launch(plan):
    """device_latest at 64 frames a launch: nothing deferred, k4_latest behind the tail on the tail's stream, the finder chain
    behind the accumulation of the batch whose back half was queued last."""
    want = dict(table=U, finder=F, accum=M, rest=M, latest=M, d2h=C, back_now=True, after=1, host_waits="none")
    assert plan(device_latest=1) == want
    assert plan(device_latest=1, slot=3, last_back=2) == dict(want, after=2)
    assert plan(device_latest=1, batch=128, last_back=5) == dict(want, after=5)


def test_no_window_below_64_frames_a_launch(plan):
    """The deferred schedule, k4_latest on a stream of its own: one for the even slots, one for the odd."""
    want = dict(table=U, finder=F, accum=M, rest=M, latest=L, d2h=C, back_now=False, after=-1, host_waits="none")
    assert plan(device_latest=1, batch=63) == want
    assert plan(device_latest=1, batch=32, slot=4) == want
    assert plan(device_latest=1, batch=32, slot=3) == dict(want, latest=L2)
    assert plan(device_latest=1, batch=32, slot=5, last_back=4) == dict(want, latest=L2)


def test_the_window_without_a_batch_before(plan):
    want = dict(table=U, finder=F, accum=M, rest=M, latest=M, d2h=C, back_now=True, after=-1, host_waits="none")
    assert plan(device_latest=1, last_back=-1) == want
    assert plan(device_latest=1, last_back=0) == dict(want, after=0)  # (slot 0 is a slot)


def test_a_timed_batch_runs_in_line(plan):
    """Everything on the main stream, the back half at once, and the host waits for the batch's copy; the finder chain on the
    main stream waits for no other batch's event, and k4_latest follows the tail there whatever the launch's width."""
    want = dict(table=M, finder=M, accum=M, rest=M, d2h=C, back_now=True, after=-1, host_waits="done_event")
    assert plan(timed=1) == want
    assert plan(timed=1, slot=3, side2=1) == want
    assert plan(timed=1, wide=0) == want and plan(timed=1, w_aside=1) == want
    assert plan(timed=1, device_latest=1) == dict(want, latest=M)
    assert plan(timed=1, device_latest=1, batch=32, slot=3) == dict(want, latest=M)


def test_one_stream(plan):
    """Every kernel of the batch on the main stream, no deferred back half, no wait on the host -- and k4_latest outside the
    window still on a stream of its own: the switch alone does not move it."""
    want = dict(table=M, finder=M, accum=M, rest=M, d2h=C, back_now=True, after=-1, host_waits="none")
    assert plan(one_stream=1) == want
    assert plan(one_stream=1, wide=0) == want and plan(one_stream=1, w_aside=1) == want and plan(one_stream=1, side2=1, slot=3) == want
    assert plan(one_stream=1, device_latest=1) == dict(want, latest=M)  # the window: behind the tail; nothing to wait for in line
    assert plan(one_stream=1, device_latest=1, batch=32) == dict(want, latest=L)
    assert plan(one_stream=1, device_latest=1, batch=32, slot=1) == dict(want, latest=L2)
    assert plan(one_stream=1, d2h_sync=1) == dict(want, host_waits="copy_stream")


def test_no_defer_only_queues_the_back_half_at_once(plan):
    assert plan(no_defer=1) == dict(plan(), back_now=True)
    assert plan(no_defer=1, device_latest=1, batch=32, slot=3) == dict(plan(device_latest=1, batch=32, slot=3), back_now=True)
    assert plan(no_defer=1)["finder"] == F and plan(no_defer=1)["table"] == U


def test_side2_moves_the_odd_slots_finder_chain(plan):
    assert plan(side2=1, slot=2) == plan(slot=2) and plan(side2=1, slot=2)["finder"] == F
    assert plan(side2=1, slot=3) == dict(plan(slot=3), finder=F2)
    assert plan(side2=1, slot=5, device_latest=1) == dict(plan(slot=5, device_latest=1), finder=F2)  # (and still waits: after)
    assert plan(side2=1, slot=5, device_latest=1)["after"] == 1


def test_w_aside_moves_the_wide_chains_chroma_launch_and_nothing_of_the_stream_chain(plan):
    want = dict(table=U, finder=F, accum=M, rest=C, d2h=C, back_now=False, after=-1, host_waits="none")
    assert plan(w_aside=1) == want
    assert plan(w_aside=1, device_latest=1) == dict(want, latest=C, back_now=True, after=1)  # k4_latest stays behind the tail
    assert plan(w_aside=1, device_latest=1, batch=32, slot=3) == dict(want, latest=L2)
    assert plan(w_aside=1, wide=0) == plan(wide=0)
    assert plan(w_aside=1, wide=0, f_serial=1) == plan(wide=0, f_serial=1)


def test_the_stream_chain_and_f_serial(plan):
    """The stream chain's chroma launch and what follows go to the copy stream unless G1S_F_SERIAL; the wide chain does not read
    that switch."""
    want = dict(table=U, finder=F, accum=M, rest=C, d2h=C, back_now=False, after=-1, host_waits="none")
    assert plan(wide=0) == want
    assert plan(wide=0, f_serial=1) == dict(want, rest=M)
    assert plan(f_serial=1) == plan()
    assert plan(wide=0, device_latest=1) == dict(want, latest=C, back_now=True, after=1)
    assert plan(wide=0, device_latest=1, batch=32) == dict(want, latest=L)


def test_luma_only_frames_have_nothing_to_move(plan):
    want = dict(table=U, finder=F, accum=M, rest=M, d2h=C, back_now=False, after=-1, host_waits="none")
    assert plan(nplanes=1) == want
    assert plan(nplanes=1, w_aside=1) == want
    assert plan(nplanes=1, wide=0) == want
    assert plan(nplanes=1, wide=0, device_latest=1, batch=32, slot=1) == dict(want, latest=L2)


def test_d2h_sync_waits_for_the_copy_stream_and_comes_first(plan):
    assert plan(d2h_sync=1) == dict(plan(), host_waits="copy_stream")
    assert plan(d2h_sync=1, timed=1) == dict(plan(timed=1), host_waits="copy_stream")
