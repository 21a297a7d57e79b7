"""tests/loop_forms.py on a CPU: the coverage the matrix claims is computed from ROWS, the model of the schedule gives hand-computed counters, and
the option ranges of the model are those hn_set_option enforces (parsed from hn_api.hip) and the header documents."""
import os
import re

import loop_forms as LF

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _facets(row):
    """What a row contributes to the pair claims, beside its side_stream value."""
    _, _, _, batch, precision, fixed, form, _, histories = row
    out = {f"deep {fixed.get('deep', 2)}", f"precision {precision}"}
    if len(LF.lane_split(batch, form["lanes"])) > 1:
        out.add("lanes > 1")
    if form["graph"] == 1:
        out.add("graph 1")
    if form["graph"] > 1:
        out.add("graph > 1")
    if "st" in histories:
        out.add("with state history")
    if not histories:
        out.add("without histories")
    return out


def test_every_value_and_every_pair_occurs():
    forms = [r[6] for r in LF.ROWS]
    assert {f["side_stream"] for f in forms} == set(range(4))
    assert {f["lanes"] for f in forms} == set(range(1, 9))
    assert {f["graph"] for f in forms} == set(LF.GRAPH_VALUES)
    assert {f["hist_copy"] for f in forms} == {0, 1} and {f["side_sync"] for f in forms} == {0, 1}
    want = {"lanes > 1", "graph 1", "graph > 1", "deep 0", "deep 1", "deep 2", "precision fp32", "precision fp16", "precision valu",
            "with state history", "without histories"}
    for ss in range(4):
        have = set().union(*[_facets(r) for r in LF.ROWS if r[6]["side_stream"] == ss])
        assert want <= have, (ss, want - have)
        assert {LF.row_class(r) for r in LF.ROWS if r[6]["side_stream"] == ss} == set("ABCDE"), ss
    assert len({r[0] for r in LF.ROWS + LF.PLAIN_ROWS}) == len(LF.ROWS) + len(LF.PLAIN_ROWS)          # tags are the test ids
    assert {LF.row_class(r) for r in LF.PLAIN_ROWS} == set("BCD") and all(r[6] == LF.PLAIN for r in LF.PLAIN_ROWS)


def test_rows_are_what_the_classes_and_the_iteration_rule_say():
    for tag, net, n, b, precision, fixed, form, n_iter, histories in LF.ROWS + LF.PLAIN_ROWS:
        cls = tag.split("_")[0]
        assert (net, n, b) == LF.CLASSES[cls], tag
        assert n % (1 << net[0]) == 0 and set(histories) <= set(LF.HISTORIES) and precision in ("fp32", "fp16", "valu"), tag
        assert set(form) == set(LF.PLAIN) and set(fixed) <= set(LF.FIXED_RANGES), tag
        for k, v in list(form.items()) + list(fixed.items()):
            if k == "graph":
                assert v in LF.GRAPH_VALUES, tag
            else:
                lo, hi = {**LF.RANGES, **LF.FIXED_RANGES}[k]
                assert lo <= v <= hi, (tag, k)
        if cls == "E":
            assert n_iter == 5 and form["lanes"] == 1 and form["graph"] == 0, tag
        elif form["graph"] == 4:
            assert n_iter == 18, tag
        else:
            assert n_iter in (9, 7) and (n_iter == 9 or form["graph"] == 2), tag
        a = LF.split_point(n_iter)
        assert a & 1 and 0 < a < n_iter, tag
    assert sum(1 for r in LF.ROWS if r[6]["graph"] == 2 and r[7] == 7) == 1
    # every (class, HN_OPT_DEEP) a row runs has its route written down
    assert {(LF.row_class(r), r[5].get("deep", 2)) for r in LF.ROWS + LF.PLAIN_ROWS} == set(LF.ROUTES)
    # the one-lane fall-back and both stand-downs of several iterations per graph are rows
    assert any(r[6]["lanes"] == 8 and r[3] == 7 for r in LF.ROWS)
    assert any(r[6]["graph"] == 2 and set(r[8]) & {"res", "wf", "st"} for r in LF.ROWS)
    # a row that is expected to replay and a row that is expected to use device words exist for every class that can
    replays = {LF.row_class(r) for r in LF.ROWS if LF.expected_counters(r[6], r[4], r[7], r[3], r[8])["graph_replays"]}
    words = {LF.row_class(r) for r in LF.ROWS if LF.expected_counters(r[6], r[4], r[7], r[3], r[8])["flag_sync_iterations"]}
    assert replays == {"A", "C"} and words >= {"A", "E"}, (replays, words)


def test_lane_split():
    assert LF.lane_split(7, 3) == [2, 2, 3]
    assert LF.lane_split(7, 8) == [7] and LF.lane_split(7, 4) == [7] and LF.lane_split(8, 4) == [2, 2, 2, 2]
    assert LF.lane_split(17, 8) == [2, 2, 2, 2, 2, 2, 2, 3]
    assert LF.lane_split(17, 5) == [3, 3, 4, 3, 4]
    assert LF.lane_split(5, 2) == [2, 3] and LF.lane_split(5, 1) == [5]
    for b in range(1, 40):
        for lanes in range(1, 9):
            s = LF.lane_split(b, lanes)
            assert sum(s) == b and min(s) >= 1 and len(s) in (1, lanes)


def _c(replays, eager, captured, words):
    return dict(zip(LF.COUNTERS, (replays, eager, captured, words)))


def test_expected_counters_by_hand():
    E, D = LF.expected_counters, LF.DEFAULT
    assert E(D, "fp32", 12, 4, ()) == _c(0, 12, 0, 11)                      # tests/test_gpu_parity.py::test_flag_sync_is_counted...
    assert E(D, "fp32", 12, 4, ("rmse",)) == _c(0, 12, 0, 11)
    assert E(D, "fp32", 1, 4, ()) == _c(0, 1, 0, 0)
    assert E(LF.form(side_sync=0), "fp32", 12, 4, ()) == _c(0, 12, 0, 0)
    assert E(D, "fp16", 12, 4, ()) == _c(0, 12, 0, 0) and E(D, "valu", 12, 4, ()) == _c(0, 12, 0, 0)
    assert E(D, "fp32", 9, 4, ("st",)) == _c(0, 9, 0, 0) and E(D, "fp32", 9, 4, ("res", "wf")) == _c(0, 9, 0, 8)
    for ss in (0, 2, 3):
        assert E(LF.form(side_stream=ss), "fp32", 9, 4, ()) == _c(0, 9, 0, 0)
    assert E(LF.PLAIN, "fp32", 1, 5, LF.HISTORIES) == _c(0, 1, 0, 0)
    # graph 4, 18 iterations: four replays of four, two left over, launched kernel by kernel with events
    assert E(LF.form(graph=4), "fp32", 18, 7, ("rmse",)) == _c(16, 2, 1, 0)
    assert E(LF.form(graph=4), "fp32", 18, 7, ("rmse",), cached=True) == _c(16, 2, 0, 0)
    assert E(LF.form(graph=4), "fp32", 15, 7, ()) == _c(0, 15, 0, 14)       # below 4 * 4: stands down, and the eager form takes the device words
    assert E(LF.form(graph=4), "fp32", 16, 7, ()) == _c(16, 0, 1, 0)
    # graph 2 with 7 iterations stands down; with 9 it replays eight; with a history it stands down
    assert E(LF.form(graph=2), "fp32", 7, 5, ()) == _c(0, 7, 0, 6)
    assert E(LF.form(graph=2), "fp32", 9, 5, ()) == _c(8, 1, 1, 0)
    assert E(LF.form(graph=2, side_stream=2), "fp32", 9, 5, ("res",)) == _c(0, 9, 0, 0)
    # graph 1 with a history still replays: the copies follow each replay
    assert E(LF.form(graph=1), "fp32", 9, 7, LF.HISTORIES) == _c(9, 0, 1, 0)
    assert E(LF.form(graph=1), "fp32", 3, 7, ()) == _c(0, 3, 0, 2) and E(LF.form(graph=1), "fp32", 4, 7, ()) == _c(4, 0, 1, 0)
    # lanes 8 with batch 7: one lane, kernel by kernel, and no device words (the option is not 1)
    assert E(LF.form(lanes=8), "fp32", 9, 7, ("rmse",)) == _c(0, 9, 0, 0)
    assert E(LF.form(lanes=8, graph=1), "fp32", 9, 7, ()) == _c(9, 0, 1, 0)
    assert E(LF.form(lanes=3, graph=1), "fp32", 9, 7, ()) == _c(0, 9, 0, 0)   # several lanes: no graph
    for r in LF.ROWS + LF.PLAIN_ROWS:         # every iteration counts exactly once
        e = E(r[6], r[4], r[7], r[3], r[8])
        assert e["graph_replays"] + e["eager_iterations"] == r[7]


def _case(src, name):
    m = re.search(r"case %s:\s*\n\s*if \(([^\n]*?)\)\s*return fail" % name, src)
    assert m, name
    return m.group(1)


def test_option_ranges_are_those_hn_set_option_enforces_and_the_header_documents():
    src = open(os.path.join(REPO, "helmnet_amd", "csrc", "hn_api.hip")).read()
    body = src.split("int hn_set_option(")[1].split("int64_t hn_get_counter(")[0]
    names = {"side_stream": "HN_OPT_SIDE_STREAM", "lanes": "HN_OPT_LANES", "hist_copy": "HN_OPT_HIST_COPY", "side_sync": "HN_OPT_SIDE_SYNC",
             "deep": "HN_OPT_DEEP", "dc_valu": "HN_OPT_DC_VALU", "dc_pair": "HN_OPT_DC_PAIR", "state_kernel": "HN_OPT_STATE_KERNEL"}
    for key, (lo, hi) in {**LF.RANGES, **LF.FIXED_RANGES}.items():
        cond = _case(body, names[key])
        m = re.fullmatch(r"value < (\d+) \|\| value > (\d+)", cond)
        assert m and (int(m.group(1)), int(m.group(2))) == (lo, hi), (key, cond)
    g = _case(body, "HN_EXP_GRAPH")
    assert g == "value < 0 || value > %d || (value > 1 && (value & 1))" % LF.GRAPH_MAX, g
    assert all(v in (0, 1) or (v % 2 == 0 and v <= LF.GRAPH_MAX) for v in LF.GRAPH_VALUES)
    # the defaults of the model are hn_create's
    internal = open(os.path.join(REPO, "helmnet_amd", "csrc", "hn_internal.h")).read()
    for key, field in (("side_stream", "opt_side_stream"), ("lanes", "opt_lanes"), ("graph", "opt_graph"), ("hist_copy", "opt_hist_copy"),
                       ("side_sync", "opt_side_sync")):
        m = re.search(r"\bint %s = (\d+)[;,]" % field, internal)
        assert m and int(m.group(1)) == LF.DEFAULT[key], (key, m and m.group(0))
    # the rules expected_counters restates are in the header
    hdr = " ".join(open(os.path.join(REPO, "include", "helmnet_hip.h")).read().split())
    hdr = hdr.replace(" * ", " ")
    for text in ("batch < 2 lanes runs as ONE lane", "[batch j / lanes, batch (j + 1) / lanes)", "only in a call of at least 4 n iterations",
                 "replays floor(n_iter / n) graphs and launches the left-over iterations kernel by kernel",
                 "when the call has a res_hist, wf_hist or st_hist", "with HN_OPT_LANES > 1 (also where a small batch runs as one lane)",
                 "in the 16-bit and HN_PREC_FP32_VALU modes, with a st_hist", "n_iter - 1 per eligible call"):
        assert text in hdr, text
    from helmnet_amd import _lib
    assert set(names) | {"graph"} <= set(_lib.HN_OPTION) and set(LF.COUNTERS) <= set(_lib.HN_COUNTER)
