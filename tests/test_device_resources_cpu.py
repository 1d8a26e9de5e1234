"""The owners of the host library's device resources (csrc/device_resources.hpp) on the CPU:
DeviceBuffer, PinnedBuffer and Event free exactly what they hold, exactly once -- in reset(), in
the destructor and under move-assignment -- so that capi.cpp's state is torn down by assigning a
fresh one, and reserve() grows as the hand-written grow() did (no call when the size fits, the
contents dropped otherwise, empty after a failure). Built with g++ from the product header against
counting stand-ins of the HIP calls, under the address and undefined-behaviour sanitizers: a
double free or a leak fails the run."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("devres") / "device_resources_driver")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "vulkancomputeraytracing_amd", "csrc"),
                    "-I", os.path.join(ROCM, "include"), "-D__HIP_PLATFORM_AMD__",
                    os.path.join(ROOT, "tests", "device_resources_driver.cpp"), "-o", exe],
                   check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stderr  # the sanitizers' verdict
    return {l.split()[0]: [int(v) for v in l.split()[1:]] for l in run.stdout.splitlines()}


@pytest.mark.parametrize("kind", ["device", "pinned"])
def test_buffer(cases, kind):
    c = {k[len(kind) + 1:]: v for k, v in cases.items() if k.startswith(kind + "_")}
    # reserve(0) on an empty buffer: success, no call, still null, capacity 0
    assert c["reserve_zero"] == [0, 0, 0, 1, 0]
    # reserve(8), (4), (8): one allocation, no free, the same pointer, capacity 8
    assert c["reserve_8_4_8"] == [1, 0, 1, 8]
    # reserve(16) after that: success, one allocation and one free, capacity 16, one live
    assert c["reserve_16"] == [0, 1, 1, 16, 1]
    # a failed reserve: the error, (one attempt, the old one freed,) null, capacity 0, none live
    assert c["reserve_fails"] == [1, 1, 1, 1, 0, 0]
    # ... and a later reserve succeeds: one allocation, no free, capacity 4
    assert c["reserve_after_failure"] == [0, 1, 0, 1, 4]
    # an empty buffer move-assigned onto a full one: exactly one free, null, none live
    assert c["move_assign_empty"] == [0, 1, 1, 0]
    # move construction: no call, the source empty, the target holds the pointer and capacity
    assert c["move_construct"] == [0, 0, 1, 1, 8]
    # a full buffer move-assigned onto a full one: the target's allocation is freed, once
    assert c["move_assign_full"] == [0, 1, 1, 1]
    # reset twice: one free
    assert c["reset_twice"] == [0, 1, 0]
    # the destructors free what is left (one buffer), nothing twice, nothing stays
    assert c["scope_end"] == [0, 1, 0]


def test_event(cases):
    c = {k[len("event_"):]: v for k, v in cases.items() if k.startswith("event_")}
    assert c["empty"] == [1]
    # create() twice: success, one hipEventCreate, none with flags, no destroy, the same event
    assert c["create_twice"] == [0, 1, 0, 0, 1]
    # create(hipEventDisableTiming): one creation, through hipEventCreateWithFlags
    assert c["create_flags"] == [0, 1, 1, 1]
    # a failed creation leaves it empty and returns the error; a later one succeeds
    assert c["create_fails"] == [1, 1, 1]
    assert c["create_after_failure"] == [0, 1, 1]
    # an empty event move-assigned onto a created one: one destroy (two others stay live)
    assert c["move_assign_empty"] == [0, 1, 1, 2]
    assert c["move_construct"] == [0, 0, 1, 1]
    assert c["reset_twice"] == [0, 1, 1]
    assert c["scope_end"] == [0, 1, 0]


def test_struct_of_owners_assigned_from_fresh(cases):
    # five resources held; the assignment allocates nothing, frees the five, leaves none live
    # and resets the scalar; the struct's own destructor then has nothing to free
    assert cases["struct_assign_fresh"] == [5, 0, 5, 0, 0]
    assert cases["struct_scope_end"] == [0, 0, 0]
