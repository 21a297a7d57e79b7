"""The forms of the hn_step loop -- which kernel runs when, on which stream and on which buffers -- as a matrix of rows, and a model of the schedule
each form must take.  Pure Python: nothing here touches the GPU (tests/test_loop_forms_host.py checks the matrix and the model on a CPU,
tests/test_loop_forms_gpu.py runs every row).

A FORM is a dict over the scheduling knobs only: ``side_stream`` 0..3, ``lanes`` 1..8, ``graph`` in {0, 1, 2, 4}, ``hist_copy`` 0/1, ``side_sync`` 0/1.
The knobs that choose kernels (``deep``, ``dc_valu``, ``dc_pair``, ``state_kernel``) are a row's FIXED options: the same in the form under test and
in its reference.  PLAIN is the form without a side stream, capture, zero-copy history slots or deferred join, driven as n_iter calls of one
iteration each; every other row must give its bits.

A ROW is (tag, network, n, batch, precision, fixed, form, n_iter, histories):
  network     (depth, weight seed, slope plan, activation, state_depth) for tests/config_weights.config_weights
  precision   'fp32' | 'fp16' | 'valu'
  histories   subset of ('res', 'wf', 'st', 'rmse'): the optional outputs the call asks for

Shape classes (the smallest shapes at which each route exists):
  A  256^2, depth 4, batch 7   paired level-0 launch, k_deepx over two levels, streaming conv_state, flag words; lanes 3 = 2 + 2 + 3, lanes 8 = one lane
  B  d3_128, batch 5           k_deep32 (the per-sample deep kernel; HN_OPT_DEEP 1, see ROUTES), no paired launch
  C  96^2, depth 4, batch 5    no deep kernel at all, every level layer by layer, release by event
  D  d2_64, batch 17           many lanes, cheap: lanes 8 = 2 x 7 + 3, lanes 5 = 3, 3, 4, 3, 4
  E  512^2, depth 4, batch 2   k_deepx over one level (side_stream rows only, 5 iterations)

Iteration counts: 9 for the eager forms and graph 1 / 2 (odd: the states end in the library's buffer and are copied back; 9 >= 4 * 2 with one
iteration left over), 18 for graph 4 (sixteen replayed, two left over), 7 once under graph 2 (below 4 * 2: the form must stand down).
"""

RANGES = {"side_stream": (0, 3), "lanes": (1, 8), "hist_copy": (0, 1), "side_sync": (0, 1)}
GRAPH_VALUES = (0, 1, 2, 4)          # of the legal ones: 0, 1 or an even number <= GRAPH_MAX
GRAPH_MAX = 64
FIXED_RANGES = {"deep": (0, 2), "dc_valu": (0, 4), "dc_pair": (0, 1), "state_kernel": (0, 1)}
HISTORIES = ("res", "wf", "st", "rmse")
COUNTERS = ("graph_replays", "eager_iterations", "graphs_captured", "flag_sync_iterations")

PLAIN = {"side_stream": 0, "lanes": 1, "graph": 0, "hist_copy": 1, "side_sync": 0}
DEFAULT = {"side_stream": 1, "lanes": 1, "graph": 0, "hist_copy": 0, "side_sync": 1}      # what hn_create sets

# class -> (network, n, batch)
CLASSES = {
    "A": ((4, 749, "A", "prelu", 4), 256, 7),
    "B": ((3, 751, "A", "prelu", 3), 128, 5),      # GPU_CONFIGS["d3_128"] of tests/config_weights.py
    "C": ((4, 749, "A", "prelu", 4), 96, 5),
    "D": ((2, 744, "B", "prelu", 2), 64, 17),      # GPU_CONFIGS["d2_64"]
    "E": ((4, 749, "A", "prelu", 4), 512, 2),
}
INPUT_SEED = 9300          # config_input(n, b, depth, INPUT_SEED + n, wf_scale=0.5)


def form(**kw):
    f = dict(DEFAULT)
    f.update(kw)
    return f


def lane_split(batch, lanes):
    """The sub-batches hn_step walks: one lane whenever batch < 2 * lanes, else lo[j] = batch * j // lanes."""
    if batch < 2 * lanes:
        return [batch]
    lo = [batch * j // lanes for j in range(lanes + 1)]
    return [lo[j + 1] - lo[j] for j in range(lanes)]


def expected_counters(form, precision, n_iter, batch, histories, cached=False):
    """The deltas of COUNTERS one hn_step call of this form must produce, from include/helmnet_hip.h (HN_EXP_GRAPH, HN_OPT_SIDE_SYNC, HN_OPT_LANES,
    HN_CNT_*).  ``cached``: the context has already captured a graph for exactly these buffers and options."""
    hist = any(h in histories for h in ("res", "wf", "st"))
    out = dict.fromkeys(COUNTERS, 0)
    if len(lane_split(batch, form["lanes"])) > 1:             # several lanes: every iteration launched kernel by kernel, events only
        out["eager_iterations"] = n_iter
        return out
    per_graph = form["graph"] if form["graph"] > 1 else 1
    graph = form["graph"] > 0 and n_iter >= 4 * per_graph and not (per_graph > 1 and hist)
    if graph:
        out["graph_replays"] = n_iter // per_graph * per_graph
        out["graphs_captured"] = 0 if cached else 1
    out["eager_iterations"] = n_iter - out["graph_replays"]
    # device words: HN_OPT_LANES 1 (the option, not the lanes a small batch falls back to), kernel-by-kernel launches, fp32, side stream policy 1,
    # nothing that reads the new states right behind an iteration; the last iteration of a call joins with an event
    if (not graph and form["lanes"] == 1 and form["side_stream"] == 1 and form["side_sync"] == 1 and precision == "fp32"
            and "st" not in histories):
        out["flag_sync_iterations"] = max(n_iter - 1, 0)
    return out


def _row(cls, tag, precision, fixed, f, n_iter, histories):
    net, n, b = CLASSES[cls]
    return (f"{cls}_{tag}", net, n, b, precision, dict(fixed), f, n_iter, tuple(histories))


def _rows():
    rows = []
    many = {0: 4, 1: 5, 2: 6, 3: 7}      # class D: lanes 8 beside one more count per policy -> 4 .. 8 all occur
    for ss in range(4):
        t = f"ss{ss}"
        # ---- A: the headline routes
        rows.append(_row("A", f"{t}_eager", "fp32", {"deep": 2}, form(side_stream=ss), 9, ()))
        rows.append(_row("A", f"{t}_lanes3", "fp32", {"deep": 2}, form(side_stream=ss, lanes=3), 9, ("res", "rmse")))
        rows.append(_row("A", f"{t}_graph1_hist", "fp32", {"deep": 2}, form(side_stream=ss, graph=1), 9, HISTORIES))
        rows.append(_row("A", f"{t}_graph4", "fp32", {"deep": 2}, form(side_stream=ss, graph=4), 18, ("rmse",)))
        rows.append(_row("A", f"{t}_deep1_zero_copy", "fp32", {"deep": 1}, form(side_stream=ss), 9, ("wf", "rmse")))
        rows.append(_row("A", f"{t}_deep0_events", "fp32", {"deep": 0}, form(side_stream=ss, side_sync=0, hist_copy=1), 9, ("res",)))
        # ---- B: the per-sample deep kernel; fp16
        rows.append(_row("B", f"{t}_fp16_sthist", "fp16", {"deep": 1}, form(side_stream=ss), 9, ("st", "rmse")))
        rows.append(_row("B", f"{t}_lanes2", "fp32", {"deep": 1}, form(side_stream=ss, lanes=2), 9, HISTORIES))
        # ---- C: no deep kernel; the direct kernels; several iterations per graph
        rows.append(_row("C", f"{t}_valu", "valu", {"deep": 2}, form(side_stream=ss), 9, ("rmse",)))
        rows.append(_row("C", f"{t}_graph2", "fp32", {"deep": 2}, form(side_stream=ss, graph=2), 9, ()))
        # ---- D: many lanes
        rows.append(_row("D", f"{t}_lanes8", "fp32", {"deep": 2}, form(side_stream=ss, lanes=8), 9, ("rmse", "st")))
        rows.append(_row("D", f"{t}_lanes{many[ss]}", "fp32", {"deep": 2}, form(side_stream=ss, lanes=many[ss]), 9, ("rmse", "wf")))
        # ---- E: k_deepx over one level
        rows.append(_row("E", f"{t}_eager", "fp32", {"deep": 2}, form(side_stream=ss), 5, ("rmse",)))
    # lanes 8 on a batch of 7 falls back to one lane; graph 2 below 4 * 2 iterations stands down, graph 2 with a history too
    rows.append(_row("A", "ss1_lanes8_one_lane", "fp32", {"deep": 2}, form(lanes=8), 9, ("rmse",)))
    rows.append(_row("C", "ss1_graph2_stands_down_7", "fp32", {"deep": 2}, form(graph=2), 7, ()))
    rows.append(_row("C", "ss2_graph2_stands_down_hist", "fp32", {"deep": 2}, form(side_stream=2, graph=2), 9, ("res",)))
    return rows


ROWS = _rows()
# the plain form against float64: the classes a CPU can loop in float64
PLAIN_ROWS = [_row(cls, "plain", "fp32", {"deep": 1 if cls == "B" else 2}, dict(PLAIN), 9, HISTORIES) for cls in ("B", "C", "D")]

# (class, HN_OPT_DEEP) -> (kernels the fp32 mode must reach, kernels it must not reach), as Engine.kernel_name spells them: the routes the classes are
# there for.  With HN_OPT_DEEP 2 a network whose last two levels are 64^2 and 32^2 takes k_deepx (so does d3_128): class B runs with 1, which
# is the per-sample kernel k_deep32 on the 32^2 level alone and leaves conv_signal_1 a launch of its own.
ROUTES = {
    ("A", 2): ({"inc_conv_signal0", "deep"}, {"conv_signal2", "conv_signal3", "bottleneck"}),
    ("A", 1): ({"inc_conv_signal0", "conv_signal2", "deep"}, {"conv_signal3", "bottleneck"}),
    ("A", 0): ({"inc_conv_signal0", "conv_signal3", "bottleneck"}, {"deep"}),
    ("B", 1): ({"conv_signal0", "conv_signal1", "deep"}, {"inc_conv_signal0", "conv_signal2", "bottleneck"}),
    ("C", 2): ({"conv_signal0", "conv_signal1", "conv_signal2", "conv_signal3", "bottleneck"}, {"inc_conv_signal0", "deep"}),
    ("D", 2): ({"conv_signal0", "deep"}, {"inc_conv_signal0", "conv_signal1", "bottleneck"}),
    ("E", 2): ({"inc_conv_signal0", "conv_signal2", "deep"}, {"conv_signal3", "bottleneck"}),
}


def row_class(row):
    return row[0].split("_")[0]


def split_point(n_iter):
    """a of the a + b split: odd (the first call ends with the states in the library's buffer and must copy them back), near the middle."""
    a = n_iter // 2
    return a if a & 1 else a + 1
