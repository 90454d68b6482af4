"""No GPU: the optimizer kernels' register budget, read from the compiler's report of the last build (build/resource_usage.txt,
written by `make`; the test skips when there has been no build here).

Span 1 may hold 240 vector registers: it then still shares a SIMD (512) with another span-1 wavefront, with span 2 (at most 256,
two wavefronts by its launch bounds) and with span 3 (272 allocated).  Nothing in these kernels may spill to scratch -- a spilled
value comes back with an exposed memory latency in every optimizer round.

Figures of the build this test came with (VGPRs, or VGPRs + AGPRs; no scratch anywhere):
  span 1, per-span, gate classes 0..4: 238 / 212 / 212 / 216 / 216 (the commit before: 226 / 200 / 200 / 204 / 204)
  span 3, per-span, gate classes 0..4: 256 + 16 / 10 / 10 / 16 / 14.  Class 3 (CNOT) was at 256 + 18 = 274 (280 allocated) in the
  commit before; minimize_kernel<3, GC_CX, false> is now held to 272 by a register cap of its own (slam_kernels.hpp) and keeps two
  lane constants in 12 bytes of scratch per lane.  The other span-3 kernels are that commit's device code.
"""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = os.path.join(ROOT, "build", "resource_usage.txt")

# _ZN7slamdev15minimize_kernelILi<K>ELi<GC>ELb<MQ>EEE...
NAME = re.compile(r"Function Name: (_ZN7slamdev15minimize_kernelILi(\d+)ELi(\d+)ELb([01])EEE\S*)")
FIELD = re.compile(r":\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]): (\d+)")


def _kernels():
    """[(name, span, multi_queue, {field: value})] of every minimize_kernel<K, GC, MQ> in the report."""
    out, cur = [], None
    for line in open(REPORT):
        m = NAME.search(line)
        if m:
            cur = (m.group(1), int(m.group(2)), m.group(4) == "1", {})
            out.append(cur)
            continue
        if "Function Name:" in line:
            cur = None
            continue
        f = FIELD.search(line)
        if cur is not None and f:
            cur[3][f.group(1)] = int(f.group(2))
    return out


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(REPORT):
        pytest.skip("no build/resource_usage.txt: nothing has been built in this tree")
    ks = _kernels()
    assert ks, "the report names no minimize_kernel: has the kernel been renamed?"
    for name, _, _, fields in ks:
        assert set(fields) == {"VGPRs", "AGPRs", "ScratchSize [bytes/lane]"}, name
    return ks


def test_span1_stays_inside_240_registers(kernels):
    span1 = [k for k in kernels if k[1] == 1 and not k[2]]
    assert len(span1) >= 5  # one per gate structure class
    for name, _, _, f in span1:
        assert f["VGPRs"] <= 240 and f["AGPRs"] == 0 and f["ScratchSize [bytes/lane]"] == 0, (name, f)


def test_span2_does_not_spill(kernels):
    span2 = [k for k in kernels if k[1] == 2]
    assert span2
    for name, _, _, f in span2:
        assert f["ScratchSize [bytes/lane]"] == 0, (name, f)


def test_span3_still_pairs_with_span1(kernels):
    span3 = [k for k in kernels if k[1] == 3 and not k[2]]
    assert span3
    for name, _, _, f in span3:
        assert f["VGPRs"] + f["AGPRs"] <= 272, (name, f)
