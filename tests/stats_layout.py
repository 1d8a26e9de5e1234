"""The layout of vcrt_stats.debug[] as the tests read it: one table, checked against the sources
by tests/test_stats_layout_cpu.py (the reg enum of csrc/tracer.hip, capi.cpp's kRegionCount and
kRegionDebugBase, and the labels tools/phases_report.py prints), used by
tests/test_gpu_stats_builds.py. A stats kernel (VCRT_DEBUG_STATS=1) writes debug[0..39] at the end
of trace_impl (tracer.hip, "if constexpr (kStats)" after the persistent loop) and the host adds the
waves' region rows into debug[40..127] (capi.cpp trace_frame)."""

# debug[] indices below the region counters: name -> index (tracer.hip, end of trace_impl)
DEBUG = {
    "wave_iters": 0,         # st_iters: loop iterations with a live lane, summed over the waves
    "live_lanes": 1,         # st_active: lanes not done, summed over those iterations
    "waves": 7,              # one per wave
    "cam_entries": 24,       # pt.cam_entries: wave entries into the camera fast trace
    "cam_lanes": 25,         # pt.cam_lanes: camera rays it traced
    "cam_live": 26,          # pt.cam_live: lanes active at those entries
    "list_trips": 27,        # pt.list_trips: listed-pair loop trips, per entry the busiest lane's
    "list_sum": 28,          # pt.list_sum: the same summed over the lanes
    "root_trips": 29,        # pt.root_trips: candidate-root loop trips, the busiest lane's
    "root_sum": 30,          # pt.root_sum: the same summed over the lanes
    "main_hit_lanes": 31,    # pt.shade_hits: main-scan lanes that hit a sphere
    "retire_ticks": 32,      # pt.retire: wave clock in the retire
    "fetch_iters": 33,       # pt.fetch_iters: wave-iterations that ran the fetch loop
    "block_fetches": 34,     # pt.blk_fetches: blocks of 64 items taken from the queues
    "items_started": 35,     # pt.items_cur: items handed to lanes (fetched or stolen)
    "group_pass_entries": 36,  # pt.group_entries: the LDS-table kernel's group-pass entries
    "node_pass_entries": 37,   # pt.node_entries: the LDS-table kernel's node-pass entries
    "retire_iters": 38,      # pt.retire_iters: wave-iterations that retired a quantum
    "quanta_retired": 39,    # pt.quanta: quanta retired, lanes
}

REGION_DEBUG_BASE = 40  # capi.cpp kRegionDebugBase
REGION_COUNT = 88       # capi.cpp kRegionCount == tracer.hip reg::kCount

# the reg:: names the tests read -> their value in the enum (tracer.hip namespace reg)
REGIONS = {
    "kIter": 0, "kRetire": 1, "kRetireNan": 2, "kRetireRing": 3, "kRetireGlobal": 4,
    "kBlock": 7, "kItem": 9, "kCam": 10, "kCamListTrip": 16, "kCamRootTrip": 17, "kScan": 19,
    "kScanLinear": 20, "kLevelNodes": 28,
    "kSteal": 37, "kLevelGroups": 78, "kSliceGroups": 83,
}

# tools/phases_report.py on a stats JSON with debug[k] = k + 1 (so wave-iters = 1 and the wave
# time debug[14] = 15): for each of debug[32..39] a regular expression that ties the label printed
# to the value of the quantity the kernel writes there.
PHASES_REPORT_LABELS = {
    32: r"retire 220\.0% of wave time \(33\.0 ticks per wave-iter\)",
    33: r"fetch loop in 34\.00 of wave-iters",
    34: r"blocks 35\.0000",
    35: r"items started 36\.000",
    36: r"group-pass entries 37\.000",
    37: r"node-pass entries 38\.000",
    38: r"run in 39\.00 of wave-iters",
    39: r"40\.00 quanta per wave-iter",
}


def dbg(st, name):
    """debug[] entry `name` of a stats() dict."""
    return st["debug"][DEBUG[name]]


def region(st, name):
    """The region counter reg::`name` of a stats() dict, summed over the waves."""
    return st["debug"][REGION_DEBUG_BASE + REGIONS[name]]
