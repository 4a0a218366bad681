"""GPU: every tensor operand of every swept entry point of PCONV.py is refused, or gives the same bits
(tests/operand_cases.py: the table, the deformations, the harness; its teeth: tests/test_operands_cpu.py).

One test id per (entry, operand, deformation).  `strided` and `offset` run for real -- their storage covers a dense read of
the operand's shape by construction -- and are held to the outcome the table pins: the bits of the call with the dense
operand (int32 views: -0 and NaN payloads count; the gaps of the buffer behind an in-place operand keep their sentinel),
or a PconvError.  `dtype`, `device` and `short` run with PCONV.call, PCONV._backward_call and _native.call replaced by a
recorder that fails the test with "reached the library with a refused operand: <entry>, <operand>, <deformation>": they
never launch anything.  Every call gets fresh ops (step counters, iteration counters, caches)."""
import time

import pytest
import torch

import operand_cases as OC

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RUN = OC.cases()[0]


@pytest.mark.parametrize("case", RUN, ids=OC.case_id)
def test_operand_is_refused_or_gives_the_same_bits(hip_backend, monkeypatch, case):
    r, o, deformation = case
    start = time.perf_counter()
    try:
        OC.check(hip_backend, r, o, deformation, DEV, "cpu", monkeypatch)
        torch.cuda.synchronize()
    except Exception as e:
        if any(s in str(e) for s in ("HIP error", "hipError", "illegal memory access")):
            pytest.exit("the GPU reported a fault in %s: nothing more is started on it: %s" % (OC.case_id(case), e), 3)
        raise
    assert hip_backend.backward_is_ordered() is False
    print("%s: %.3f s" % (OC.case_id(case), time.perf_counter() - start))
