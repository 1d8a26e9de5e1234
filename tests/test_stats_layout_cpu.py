"""The stats builds' debug[] layout (tests/stats_layout.py) against the sources that define it:
the reg enum of csrc/tracer.hip, the host's row size and base in capi.cpp, and the labels
tools/phases_report.py prints for debug[32..39]. No GPU."""
import json
import os
import re
import runpy
import sys

from tests import stats_layout as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")
CSRC = os.path.join(ROOT, "vulkancomputeraytracing_amd", "csrc")


def reg_enum():
    from tools import valu_regions  # the enum's one parser
    with open(valu_regions.TRACER) as f:
        return valu_regions.enum_values(f.read()), valu_regions.REGION_DEBUG_BASE


def test_region_table_matches_the_kernel_enum():
    enum, base = reg_enum()
    assert enum["kCount"] == 88 == L.REGION_COUNT
    assert base == L.REGION_DEBUG_BASE
    for name, value in L.REGIONS.items():
        assert enum[name] == value, name
    # the absolute regions are distinct and below kCount (the shading's kSh* are offsets from
    # kShadeBase0/1 and repeat small values by design)
    absolute = {n: v for n, v in enum.items() if not n.startswith("kSh") and n != "kCount"}
    assert len(set(absolute.values())) == len(absolute)
    assert max(absolute.values()) < enum["kCount"]
    assert L.REGION_DEBUG_BASE + L.REGION_COUNT == 128  # vcrt_stats.debug[128], to its end


def test_host_row_size_and_base():
    with open(os.path.join(CSRC, "capi.cpp")) as f:
        capi = f.read()
    with open(os.path.join(CSRC, "tracer.hip")) as f:
        tracer = f.read()
    assert int(re.search(r"constexpr uint32_t kRegionCount = (\d+);", capi).group(1)) == \
        L.REGION_COUNT
    assert int(re.search(r"constexpr uint32_t kRegionDebugBase = (\d+);", capi).group(1)) == \
        L.REGION_DEBUG_BASE
    assert int(re.search(r"constexpr uint32_t kRegions = (\d+);", tracer).group(1)) == \
        L.REGION_COUNT


def test_debug_indices_match_the_kernels_writes():
    """Each debug[] index of the table against the field trace_impl adds there."""
    with open(os.path.join(CSRC, "tracer.hip")) as f:
        tracer = f.read()
    writes = dict((int(k), v) for k, v in re.findall(
        r"atomicAdd\(P\.debug \+ (\d+), \(unsigned long long\)(?:pt\.)?(\w+)\)", tracer))
    fields = {"wave_iters": "st_iters", "live_lanes": "st_active", "cam_entries": "cam_entries",
              "cam_lanes": "cam_lanes", "cam_live": "cam_live", "list_trips": "list_trips",
              "list_sum": "list_sum", "root_trips": "root_trips", "root_sum": "root_sum",
              "main_hit_lanes": "shade_hits", "retire_ticks": "retire",
              "fetch_iters": "fetch_iters", "block_fetches": "blk_fetches",
              "items_started": "items_cur", "group_pass_entries": "group_entries",
              "node_pass_entries": "node_entries", "retire_iters": "retire_iters",
              "quanta_retired": "quanta"}
    for name, field in fields.items():
        assert writes[L.DEBUG[name]] == field, name
    assert re.search(r"atomicAdd\(P\.debug \+ 7, 1ull\);", tracer) and L.DEBUG["waves"] == 7


def test_phases_report_labels(tmp_path, monkeypatch, capsys):
    """tools/phases_report.py names debug[32..39] as what the kernel writes there."""
    st = {"debug": [k + 1 for k in range(128)], "kernel_ms": 1.0, "bound_tests": 2,
          "group_tests": 3}
    path = tmp_path / "phases.json"
    path.write_text(json.dumps(st))
    monkeypatch.setattr(sys, "argv", ["phases_report.py", str(path)])
    runpy.run_path(os.path.join(TOOLS, "phases_report.py"), run_name="__main__")
    out = capsys.readouterr().out
    assert sorted(L.PHASES_REPORT_LABELS) == list(range(32, 40))
    for k, pattern in L.PHASES_REPORT_LABELS.items():
        assert re.search(pattern, out), f"debug[{k}]: {pattern!r} not in\n{out}"
    assert "next items" not in out and "switches" not in out


def test_every_stats_symbol_has_a_gpu_case():
    """Every *_stats kernel tracer.hip defines (nine) is the expected kernel of some case of
    tests/test_gpu_stats_builds.py's table."""
    from tests.test_gpu_stats_builds import KERNELS
    with open(os.path.join(CSRC, "tracer.hip")) as f:
        defined = set(re.findall(r"__global__[^;{]*?void (vcrt_trace_\w+_stats)\(", f.read()))
    assert len(defined) == 9
    assert {k[4] + "_stats" for k in KERNELS} == defined
