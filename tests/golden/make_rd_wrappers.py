"""Records tests/golden/rd_wrappers.json: what the Python wrappers of the device-resident calls (rd.QueryRays .. rd.TraceAreaPathsTorch)
ask of the library, return and refuse, and the public surface of rd.py, by the case tables of tests/rd_wrapper_cases.py.  The file
records this project's own rd.py at the commit named in it -- the one before the wrappers were put on one argument layer -- so
that a change to that layer is held to what the wrappers did before it.  Nothing in it comes from the reference.

    python tests/golden/make_rd_wrappers.py cpu  COMMIT     # marshalling, Buffer-route refusals, CPU tensors, public surface
    python tests/golden/make_rd_wrappers.py gpu  OUT.json   # the CUDA-tensor part, on a machine with a GPU; writes OUT.json
    python tests/golden/make_rd_wrappers.py join OUT.json   # puts that part into the golden

Neither part loads librdx.so.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
GOLDEN = os.path.join(HERE, "rd_wrappers.json")
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import rd_wrapper_cases as wc  # noqa: E402


def write(doc):
    """one outcome, one group of cases, one public name per line: the file stays readable in a diff"""
    stored = wc.pack(doc)
    rows = lambda d: "{\n%s\n }" % ",\n".join("  %s: %s" % (json.dumps(k), json.dumps(d[k], sort_keys=True)) for k in sorted(d))
    with open(GOLDEN, "w") as f:
        f.write('{\n "recorded_at": %s,\n "surface": %s,\n "cpu": %s,\n "gpu": %s,\n "outcomes": [\n%s\n ]\n}\n' % (
            json.dumps(stored["recorded_at"]), rows(stored["surface"]), rows(stored["cpu"]), rows(stored["gpu"]),
            ",\n".join("  " + json.dumps(v, sort_keys=True) for v in stored["outcomes"])))


def main(argv):
    mode = argv[1]
    doc = wc.golden(GOLDEN) if os.path.exists(GOLDEN) else {}
    if mode == "join":
        doc["gpu"] = json.load(open(argv[2]))
        return write(doc)
    if mode == "gpu":
        import torch
        assert torch.cuda.is_available()
        torch.zeros(1, device="cuda").cpu()          # torch initialises the GPU first
    import rrt_amd  # noqa: F401
    from radiance_ray_tracing_amd import rd
    if mode == "cpu":
        doc["recorded_at"], doc["cpu"] = argv[2], wc.cpu_part(rd)
        write(doc)
    else:
        os.makedirs(os.path.dirname(os.path.abspath(argv[2])), exist_ok=True)
        json.dump(wc.gpu_part(rd, torch), open(argv[2], "w"))
        print("RD-WRAPPERS-RECORDED")


if __name__ == "__main__":
    main(sys.argv)
