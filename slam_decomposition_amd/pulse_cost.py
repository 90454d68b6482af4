"""Circuit cost of targets under a set of basis gates, without optimisation (reference: ``TemplateOptimizer.cost_target_U`` /
``cost_from_distribution``, src/slam/optimizer.py:156-178).

For a ``MixedOrderBasisCircuitTemplate`` a target costs what the cheapest coverage entry whose region contains it costs
(polytope_wrap.py:39-94, basis.py:321-326).  Over a distribution of targets that is a histogram: how many targets each entry is the
first to contain.  ``slam_coverage_lookup`` builds it on the device -- the targets and their Weyl coordinates stay there -- for one or
several gate sets in one launch, and the total is summed here, in cost order, from the integer counts (bit-for-bit reproducible).

Decisions where the reference's behaviour is an accident:
  * a local target costs 0 (the reference's ``unit_cost`` returns whichever entry was bound before, or None);
  * an empty sampler costs 0.0 (the reference raises UnboundLocalError);
  * a target no entry contains raises ``ValueError("Monodromy did not find a polytope containing U ...")`` for the whole call: the
    coverage set stops at ``maximum_span_guess`` gates, where the reference's grows until it covers the chamber.
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np

from . import runtime

TOL = 1e-7  # CircuitCoverage.inside: span_rules._TOL + its default slack (8e-8)
_UNREACHABLE = "Monodromy did not find a polytope containing U"  # polytope_wrap.py:91-93


def unreachable_error(template) -> ValueError:
    return ValueError(f"{_UNREACHABLE} (the coverage set ends at maximum_span_guess = {int(template.maximum_span_guess)} gates: "
                      "raise maximum_span_guess to reach it)")


def _check_templates(templates) -> None:
    for t in templates:
        if not getattr(t, "mixed_order", False):
            raise ValueError("use customcosttemplate to have defined costs")  # optimizer.py:171-172


def _load_targets(ctx, sampler) -> int:
    """Make the sampler's targets the resident batch of ``ctx``: generated in place for a device sampler (``DeviceHaarBatch``),
    uploaded once otherwise.  Returns their number."""
    if hasattr(sampler, "fill"):
        n = int(sampler.n_samples)
        if n:
            sampler.fill(ctx)
        return n
    targets = [np.asarray(t, dtype=np.complex128) for t in sampler]
    for t in targets:
        if t.shape != (4, 4):
            raise ValueError("targets must be 4x4 unitaries")
    if targets:
        ctx.set_targets(np.stack(targets))
    return len(targets)


def lookup_counts(templates: Sequence, sampler, device=None) -> Tuple[List[np.ndarray], int, object]:
    """Per template, int64 [n_entries + 2]: how many of the sampler's targets each coverage entry is the first to contain, then local
    targets, then targets no entry contains -- all templates in ONE device launch.  Returns ``(counts, n_targets, ctx)``."""
    templates = list(templates)
    _check_templates(templates)
    if not templates:
        raise ValueError("no templates")
    ctx = runtime.get_context(templates[0].device if device is None else device)
    n = _load_targets(ctx, sampler)
    if n == 0:
        return [np.zeros(len(t.coverage) + 2, dtype=np.int64) for t in templates], 0, ctx
    counts, _ = ctx.coverage_lookup([t.coverage_table() for t in templates], 0, n, tol=TOL)
    return counts, n, ctx


def total_cost(template, counts: np.ndarray) -> float:
    """``sum_e count_e * cost_e`` in cost order (local targets cost 0); raises if some target is out of reach of every entry."""
    costs = template.coverage_table().costs
    if int(counts[len(costs) + 1]) > 0:
        raise unreachable_error(template)
    total = 0.0
    for c, k in zip(costs.tolist(), counts[: len(costs)].tolist()):
        total += k * c
    return total


def cost_sweep(templates: Sequence, sampler, device=None) -> List[float]:
    """Total circuit cost of the sampler's targets under each mixed-order template (``TemplateOptimizer.cost_from_distribution`` per
    template), from one ``slam_coverage_lookup`` over the resident targets: their Weyl coordinates are computed once for the sweep."""
    counts, _, _ = lookup_counts(templates, sampler, device)
    return [total_cost(t, c) for t, c in zip(templates, counts)]
