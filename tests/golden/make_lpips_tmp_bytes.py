"""Writes tests/golden/lpips_tmp_bytes.json: what dgs_lpips_{alex,vgg,squeeze}_tmp_bytes return and what
dgs_last_error() says after a fixed list of refused calls, recorded from the library as it stood BEFORE the three plan
functions and drivers of csrc/lpips.hip became one (commit 5b928f7).  tests/test_lpips_plan_host.py holds the library
of the tree to these numbers and texts, so the file is never regenerated from the code it pins:

    git worktree add ../parent 5b928f7 && (cd ../parent && python -m deblurgs_amd.build)
    DGS_LIB_PATH=$PWD/../parent/deblurgs_amd/libdgs_hip.so python tests/golden/make_lpips_tmp_bytes.py

Neither the sizes nor the refusals touch a device.  The test imports `NETS`, `size_cases` and `refused_calls` from here, so
both sides make the same calls.
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "lpips_tmp_bytes.json")
RECORDED_FROM = "5b928f7"
NETS = {"alex": 31, "vgg": 16, "squeeze": 17}      # the smallest image of each backbone
NS = (0, 1, 2, 3, 40, 65535, 65536)


def size_cases(net):
    """(W, H, n): every W x H of the twelve sizes for one and for three pairs, every n at nine sizes, the refusal corners."""
    m = NETS[net]
    sizes = (m - 1, m, m + 1, 33, 64, 200, 255, 256, 257, 1079, 1080, 1920)
    cases = [(W, H, n) for n in (1, 3) for W in sizes for H in sizes]
    for W, H in ((m, m), (m + 1, m - 1), (33, 64), (200, 255), (257, 256), (64, 200), (1079, 1080), (1920, 1080), (1080, 1920)):
        cases += [(W, H, n) for n in NS]
    return cases + [(65536, m, 1), (65537, m, 1), (m, 65536, 1), (32768, 32768, 1)]


def _struct_type(net):
    from deblurgs_amd import _lib
    return {"alex": _lib.DgsLpipsAlexWeights, "vgg": _lib.DgsLpipsVggWeights, "squeeze": _lib.DgsLpipsSqueezeWeights}[net]


def refused_calls(net):
    """[(label, args, keep)]: args = (a, b, n_pairs, W, H, weights, tmp, out, stream) of a call that is refused before any
    HIP call.  Every non-null pointer is the address of 256 host bytes that are never read; `keep` holds what args point
    to."""
    m = NETS[net]
    dummy = ctypes.create_string_buffer(256)
    a = ctypes.cast(dummy, ctypes.c_void_p)
    T = _struct_type(net)
    slots = ctypes.sizeof(T) // ctypes.sizeof(ctypes.c_void_p)      # 15, 31, 57

    def weights(hole=None):
        w = T()
        flat = ctypes.cast(ctypes.pointer(w), ctypes.POINTER(ctypes.c_void_p))
        for i in range(slots):
            flat[i] = None if i == hole else a.value
        return w

    def call(label, n=1, W=m, H=m, a0=a, hole=None):
        w = weights(hole)
        return label, (a0, a, n, W, H, ctypes.byref(w), a, a, None), (dummy, w)

    return ([call("null image", a0=None)] +
            [call(f"null weight in slot {i} of {slots}", hole=i) for i in (0, slots // 2, slots - 1)] +
            [call("n_pairs 0", n=0), call("n_pairs 65536", n=65536), call("W below the minimum", W=m - 1),
             call("H below the minimum", H=m - 1)])


def record(L, net):
    q = getattr(L, f"dgs_lpips_{net}_tmp_bytes")
    f = getattr(L, f"dgs_lpips_{net}")
    refused = []
    for label, args, _keep in refused_calls(net):
        rc = f(*args)
        refused.append({"call": label, "rc": rc, "error": L.dgs_last_error().decode()})
    return {"tmp_bytes": [[W, H, n, q(W, H, n)] for W, H, n in size_cases(net)], "refused": refused}


def main():
    if not os.environ.get("DGS_LIB_PATH"):
        sys.exit("set DGS_LIB_PATH to a library built from commit %s: this file is not made from the tree's own library"
                 % RECORDED_FROM)
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from deblurgs_amd import _lib
    L = _lib.lib()
    doc = {"recorded_from": RECORDED_FROM}
    doc.update({net: record(L, net) for net in NETS})
    with open(OUT, "w") as fh:
        json.dump(doc, fh, separators=(",", ":"))
        fh.write("\n")
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
