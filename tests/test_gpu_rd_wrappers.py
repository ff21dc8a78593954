"""GPU suite (-m gpu): the torch route of the device-resident calls, rd.QueryRaysTorch .. rd.TraceAreaPathsTorch, on CUDA tensors, held
to what it did at the commit named in tests/golden/rd_wrappers.json: every refusal of a tensor of a wrong dtype, trailing shape, row
count, stride or device and of a non-tensor as a whole string, the other arguments' refusals, the returned structure for 0 rows, and
for 3 rows the rdx_buffer_wrap calls (sizes, and which tensor each address belongs to) and the library call behind them.  A stand-in
records in the place of the library (tests/rd_wrapper_cases.py): no librdx.so is loaded, no scene is built.  The per-call GPU tests
hold the results of both routes; this one holds the texts and shapes they do not look at."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CHILD = r"""
import json, os, sys
ROOT = sys.argv[1]
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch
assert torch.cuda.is_available()
torch.zeros(1, device="cuda").cpu()                      # torch initialises the GPU first (tests/test_cpu_oracle._gpu_present)
import rrt_amd
from radiance_ray_tracing_amd import _lib, rd
import rd_wrapper_cases as wc
recorded = wc.golden(os.path.join(ROOT, "tests", "golden", "rd_wrappers.json"))["gpu"]
replayed = json.loads(json.dumps(wc.gpu_part(rd, torch)))
first, count = wc.differences(replayed, recorded)
assert count == 0, "%d cases differ from the golden:\n%s" % (count, "\n".join(first))
cases = recorded["cases"]
for name in wc.TORCH_ROUTE:
    zero = [v for k, v in cases.items() if k.startswith("torch/%s/" % name) and k.endswith("n=0")]
    three = [v for k, v in cases.items() if k.startswith("torch/%s/" % name) and k.endswith("n=3")]
    refused = [v for k, v in cases.items() if k.startswith("torch-refuse/%s/" % name) and "refused" in v]
    # 0 rows never reach the library; AccumulateTorch has wrapped its frame tensors by then
    assert zero and all("returned" in v and (v["calls"] == [] or (name == "AccumulateTorch" and all(c.startswith("rdx_buffer_wrap(") for c in v["calls"]))) for v in zero), name
    assert three and all("returned" in v for v in three), name
    assert sum(bool(v["calls"]) and not v["calls"][-1].startswith("rdx_buffer_wrap(") for v in three) >= len(three) - 2, name       # AccumulateTorch: two frames of no pixels
    assert len(refused) >= 10, name
assert _lib._lib is None, "librdx.so was loaded"
print("RD-WRAPPERS-OK", len(cases))
"""


def test_the_torch_route_is_the_recorded_one(gpu):
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", _CHILD, ROOT]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0 and "RD-WRAPPERS-OK" in out.stdout, (out.stdout[-2000:], out.stderr[-6000:])
