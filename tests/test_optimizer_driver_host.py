"""CPU: what ``TemplateOptimizer``'s ``_run_batch*`` strategies ask of their contexts, pinned call by call.

Every case of ``fake_ctx.CASES`` runs one strategy against recording stand-in contexts (``tests/fake_ctx.py``: no library, no GPU) and
is compared for exact equality with ``tests/golden/optimizer_driver_transcripts.json`` -- the transcript of every context (method,
scalars, arrays by value or digest, every ``OptParams`` field), the three returned arrays or the exception, ``_span_losses``,
``last_stats`` and ``last_stats_per_device``.  The file was recorded by ``tools/make_driver_transcripts.py`` before the strategies'
shared steps (context preparation, thread fan-out, merge rule, span limit) were put into helpers; it is the project's own recorded
behaviour, as ``bfgs_port_pinned.json`` is.  The tests below the comparison spell out the pins a reader would look for."""
import json
import os

import numpy as np
import pytest

import fake_ctx
from slam_decomposition_amd import _ffi

with open(os.path.join(os.path.dirname(__file__), "golden", "optimizer_driver_transcripts.json")) as f:
    GOLDEN = json.load(f)

_RUNS = {}


def run(name):
    """(result, book) of a case, run once per session."""
    if name not in _RUNS:
        _RUNS[name] = fake_ctx.CASES[name]()
    return _RUNS[name]


def calls(result, ctx, method):
    return [args for name, args in result["transcripts"][ctx] if name == method]


def values(encoded):
    return np.array(encoded["v"], dtype=encoded["dtype"]).reshape(encoded["shape"])


def test_the_fixture_holds_exactly_the_cases():
    assert sorted(GOLDEN) == sorted(fake_ctx.CASES)


@pytest.mark.parametrize("name", sorted(fake_ctx.CASES))
def test_strategy_matches_its_recorded_transcript(name):
    result = json.loads(json.dumps(run(name)[0]))  # (tuples -> lists, as the fixture went through JSON)
    want = GOLDEN[name]
    assert sorted(result) == sorted(want)
    assert sorted(result["transcripts"]) == sorted(want["transcripts"])
    for ctx, log in want["transcripts"].items():
        got = result["transcripts"][ctx]
        assert [c[0] for c in got] == [c[0] for c in log], ctx
        for i, (g, w) in enumerate(zip(got, log)):
            assert g == w, f"context {ctx}, call {i} ({w[0]})"
    for key in want:
        assert result[key] == want[key], key


def test_single_device_call_is_pinned_and_based_at_zero():
    result, _ = run("run_batch_one_device")
    (call,) = calls(result, "0/0", "decompose_range")
    assert call["pinned"] is True and call["params"]["target_base"] == 0 and (call["first"], call["count"]) == (0, 7)
    assert call["params"]["flags"] == _ffi.FLAG_EARLY_EXIT | _ffi.FLAG_ORDERED
    assert len(calls(result, "0/0", "fetch_span_losses")) == 1
    quiet, _ = run("run_batch_one_device_no_span_losses")
    assert calls(quiet, "0/0", "fetch_span_losses") == [] and quiet["span_losses"] is None
    loose, _ = run("run_batch_not_deterministic")
    assert calls(loose, "0/0", "decompose_range")[0]["params"]["flags"] == _ffi.FLAG_EARLY_EXIT | _ffi.FLAG_NO_OVERLAP


@pytest.mark.parametrize("name,second", [("run_batch_two_devices", "1/1"), ("run_batch_auto_shards", "0/1")])
def test_shards_use_slot_r_and_the_global_target_base_and_agree_with_one_call(name, second):
    result, _ = run(name)
    whole, _ = run("run_batch_one_device")
    a, b = calls(result, "0/0", "decompose_range")[0], calls(result, second, "decompose_range")[0]
    assert (a["count"], b["count"]) == (4, 3) and (a["params"]["target_base"], b["params"]["target_base"]) == (0, 4)
    assert a["pinned"] is False and b["pinned"] is False
    assert a["params"]["flags"] & _ffi.FLAG_NO_OVERLAP
    assert values(calls(result, second, "set_targets")[0]["index"]).tolist() == [4.0, 5.0, 6.0]
    assert result["returned"] == whole["returned"] and result["span_losses"] == whole["span_losses"]  # concatenated in target order
    per = result["last_stats_per_device"]
    assert len(per) == 2 and result["last_stats"]["total_ms"] == max(p["total_ms"] for p in per)
    assert result["last_stats"]["items"] == [x + y for x, y in zip(per[0]["items"], per[1]["items"])] == whole["last_stats"]["items"]


def test_fewer_targets_than_devices_is_one_unpinned_call_on_the_first_device():
    result, _ = run("run_batch_two_devices_one_target")
    assert list(result["transcripts"]) == ["0/0"] and calls(result, "0/0", "decompose_range")[0]["pinned"] is False


def test_a_failing_shard_is_what_the_caller_sees():
    result, _ = run("run_batch_shard_raises")
    assert result["error"] == ["RuntimeError", "shard 1 cannot run"]


def test_any_order_visits_the_open_targets_per_size():
    result, _ = run("any_order")
    first, second = calls(result, "0/0", "decompose_list")
    assert values(first["targets"]).tolist() == list(range(10)) and (first["k_min"], first["k_max"], first["k_layout"]) == (1, 1, 3)
    assert values(second["targets"]).tolist() == [t for t in range(10) if (t + 1) % 3] and (second["k_min"], second["k_layout"]) == (3, 3)
    cycles = values(result["returned"][2]).tolist()
    assert cycles == [1 if (t + 1) % 3 == 0 else 3 for t in range(10)]


def test_by_span_runs_each_size_once_and_lower_bounds_up_to_the_maximum():
    exact, _ = run("by_span_exact")
    assert [(c["k_min"], c["k_max"], values(c["targets"]).tolist()) for c in calls(exact, "0/0", "decompose_list")] == [
        (1, 1, [0, 4]), (2, 2, [1, 2]), (3, 3, [3])]
    bound, _ = run("by_span_lower_bound")
    assert [(c["k_min"], c["k_max"]) for c in calls(bound, "0/0", "decompose_list")] == [(1, 3), (2, 3), (3, 3)]


def test_mixed_order_keeps_the_entry_a_target_ended_with():
    result, _ = run("mixed_order")
    assert [values(c["targets"]).tolist() for c in calls(result, "0/0", "decompose_list")] == [[0, 2, 4], [0, 1, 3], [0, 3, 4, 5]]
    assert result["extra"]["circuit_polytopes"] == [0, 1, 0, 1, 2, 2]  # (target 0 keeps entry 0: the two-gate loss is not lower)
    assert [[j for j, _ in tried] for tried in result["extra"]["entries_tried"]] == [[0, 1, 2], [1], [0], [1, 2], [0, 2], [2]]
    quiet, _ = run("mixed_order_no_span_losses")
    assert quiet["extra"]["entries_tried"] == [[]] * 6 and quiet["returned"] == result["returned"]
    assert run("mixed_order_local_target")[0]["error"] == ["ValueError", ""]


def test_predicted_keeps_the_reference_exceptions():
    assert run("predicted_unreachable")[0]["error"] == ["ValueError", "Monodromy did not find a polytope containing U"]
    assert run("predicted_local")[0]["error"] == ["ValueError", ""]
    result, _ = run("predicted")
    assert [c[0] for c in result["transcripts"]["0/0"]][:4] == ["sample_haar", "set_gates", "set_cost", "reset_stats"]


def test_family_runs_one_list_per_member_and_size_in_pair_order():
    result, _ = run("family")
    assert [c[0] for c in result["transcripts"]["0/0"]][:3] == ["set_targets", "family.device_lookup", "set_gates"]
    got = [(c["gate_seqs"], values(c["targets"]).tolist()) for c in calls(result, "0/0", "decompose_list")]
    assert got == [([[0]], [5]), ([[0, 0]], [0, 2]), ([[1, 1, 1]], [3]), ([[2]], [1, 4])]
    assert values(result["extra"]["family_members"]).tolist() == [1, 4, 1, 2, 4, 1]
    assert values(result["extra"]["family_costs"]).tolist() == [3 * 0.125 + 2 * 0.25, 2 * 0.125 + 1.0, 0.875, 4 * 0.125 + 3 * 0.5, 1.25, 0.5]
    assert run("family_unreachable")[0]["error"] == ["ValueError", "no member of the family reaches the target"]
    assert run("family_local")[0]["error"] == ["ValueError", ""]


def test_v2_shards_run_on_fresh_contexts_that_are_closed():
    for name, method in (("v2_range_two_devices", "v2_decompose_range"), ("v2_stage_loop_two_devices", "v2_minimize_stage")):
        result, _ = run(name)
        single, _ = run(name.replace("_two_devices", ""))
        assert list(result["transcripts"]) == ["0/fresh", "1/fresh"] and list(single["transcripts"]) == ["0/0"]
        assert all(log[-1][0] == "close" for log in result["transcripts"].values())
        assert [calls(result, c, method)[0]["params"]["target_base"] for c in result["transcripts"]] == [0, 4]
        assert calls(result, "1/fresh", method)[0]["params"]["items_per_quad"] == 0
        assert result["returned"] == single["returned"] and result["span_losses"] == single["span_losses"]
    stage = calls(run("v2_stage_loop")[0], "0/0", "v2_minimize_stage")
    assert [c["want_items"] for c in stage] == [False, False] and [len(c["gate_seq"]) for c in stage] == [1, 3]


def test_v2_library_errors():
    assert run("v2_range_unsupported")[0]["error"][0] == "NotImplementedError"
    result, _ = run("v2_stage_unsupported_two_devices")
    assert result["error"][0] == "NotImplementedError" and result["transcripts"]["1/fresh"][-1][0] == "close"
    assert run("v2_other_library_error")[0]["error"][0] == "SlamHipError"


def test_callback_reruns_a_stage_once_with_room_for_the_longest_restart():
    result, _ = run("callback")
    assert [(len(c["gate_seq"]), c["trace_cap"]) for c in calls(result, "0/0", "minimize_stage_trace")] == [(1, 256), (1, 300), (2, 256), (3, 256)]
    assert result["extra"]["same_growing_list"] == [True, True, True]
    assert [len(per) for per in result["extra"]["records"]] == [1, 1, 0]  # (one entry per firing of the break condition)
    forced, _ = run("callback_override_fail")
    assert [len(per) for per in forced["extra"]["records"]] == [1, 2, 1]  # (target 1: the failed span's last restart, then the hit)
    assert forced["extra"]["same_growing_list"] == [True, True, True]
    assert run("callback_nothing_ran")[0]["error"] == ["ValueError", "empty spanning range"]


def test_host_method_prepares_its_context_and_counts_its_evaluations():
    result, book = run("host_method")
    assert [c[0] for c in result["transcripts"]["0/0"]] == ["set_targets", "set_gates", "set_cost"]
    stats = result["last_stats"]
    assert stats["evals"][1] > 0 and sum(stats["evals"]) == stats["evals"][1] and stats["kernel_launches"] == 0 and book.evals > 0


@pytest.mark.parametrize("name,text", [("run_batch_span_too_large", "(got 17)"), ("run_batch_span_too_large_any_order", "(got 17)"),
                                       ("by_span_too_large", "(got 17)"), ("callback_span_too_large", "(got 17)"),
                                       ("host_method_span_too_large", "(got 17)")])
def test_span_limit_message(name, text):
    kind, message = run(name)[0]["error"]
    assert kind == "NotImplementedError" and message == f"template spans up to 16 are implemented on the HIP path {text}"
