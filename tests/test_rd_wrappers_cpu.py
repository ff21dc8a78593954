"""CPU suite: the Python wrappers of the device-resident calls, rd.QueryRays .. rd.TraceAreaPathsTorch, held to what they did at the
commit named in tests/golden/rd_wrappers.json: the library calls of every Buffer-route wrapper in order with their arguments and
creation sizes, what it returns, every Python-level refusal as a whole string, the order of each call's checks, what the torch route
says to CPU tensors, and the signature and docstring of every public name of rd.py.  A stand-in records in the place of the library
(tests/rd_wrapper_cases.py), so no librdx.so is needed."""
import json
import os

import pytest

import rd_wrapper_cases as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rd():
    import rrt_amd  # noqa: F401
    from radiance_ray_tracing_amd import rd
    return rd


@pytest.fixture(scope="module")
def recorded():
    return wc.golden(os.path.join(ROOT, "tests", "golden", "rd_wrappers.json"))["cpu"]


@pytest.fixture(scope="module")
def replayed(rd):
    return json.loads(json.dumps(wc.cpu_part(rd)))


def test_the_stand_in_is_gone_after_a_case(rd):
    real = rd._lib.lib
    with wc.stand_in(rd) as rec:
        assert rd._lib.lib() is rec and rec.rdx_buffer_create(4) == 1001 and rec.calls == [["rdx_buffer_create", 4]]
    assert rd._lib.lib is real


def test_the_tables_cover_every_wrapper(rd, recorded):
    cases = recorded["cases"]
    assert len(wc.BUFFER_ROUTE) == len(wc.TORCH_ROUTE) == 14
    for name in wc.BUFFER_ROUTE:
        accepted = [v for k, v in cases.items() if k.startswith("marshal/%s/" % name)]
        refused = [v for k, v in cases.items() if k.startswith("refuse/%s/" % name) and "refused" in v]
        assert len(accepted) >= 5 and all("returned" in v and v["calls"] for v in accepted), name
        assert len(refused) >= 5 and not any(v["calls"] for v in refused), name         # every output is given: no refusal hides behind a creation
        assert accepted[0]["calls"][-1].startswith("rdx_") and "Torch" not in name
        order = cases["order/%s" % name]["returned"]
        assert len(order) >= 3 and order[-1][0] in ("still wrong: ", "still wrong: n"), name        # every check was reached
    for name in wc.TORCH_ROUTE:
        assert any(k.startswith("cpu-tensors/%s/" % name) and "must be a contiguous" in v.get("refused", "") for k, v in cases.items()), name
    assert set(wc.BUFFER_ROUTE + wc.TORCH_ROUTE) <= set(recorded["surface"])


def test_marshalling_refusals_and_cpu_tensors_are_the_recorded_ones(replayed, recorded):
    first, count = wc.differences({"cases": replayed["cases"]}, {"cases": recorded["cases"]})
    assert count == 0, "%d cases differ from the golden:\n%s" % (count, "\n".join(first))
    assert len(recorded["cases"]) >= 500


def test_the_public_surface_is_the_recorded_one(replayed, recorded):
    first, count = wc.differences({"surface": replayed["surface"]}, {"surface": recorded["surface"]})
    assert count == 0, "%d public names differ from the golden:\n%s" % (count, "\n".join(first))
