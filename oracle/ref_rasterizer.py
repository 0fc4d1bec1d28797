"""The reference rasteriser's OWN kernels on the device: build recipe and ctypes front-end.

TEST INFRASTRUCTURE ONLY, like oracle/oracle.py: imported by tests/ and ``__graft_entry__.build()``, never by the
product package ``deblurgs_amd``.

Recipe (``build_ref``).  The reference's three translation units (cuda_rasterizer/forward.cu, backward.cu,
rasterizer_impl.cu) use nothing HIP lacks, so they are compiled for gfx950 as they stand:

  1. cuda_rasterizer/*.cu and *.h are copied to a temporary directory outside the repository;
  2. the copies get the mechanical edits of ``EDITS`` (clang does not accept the spaced kernel-launch brackets), nothing else;
  3. hipcc compiles them with ``FLAGS``, against the shim headers of oracle/refshim/ (include forwarding and renames only),
     the copies and the reference's vendored third_party/glm;
  4. they are linked with oracle/ref_rasterizer_wrap.cpp (C entry points, the project's own text);
  5. the temporary copies are deleted.

Twice, mirroring the oracle's two builds: oracle/_ref/libdgs_refkernels_f32.so (-ffp-contract=off) and
oracle/_ref/libdgs_refkernels_fma.so (-ffp-contract=fast, what nvcc's default --fmad=true does to the reference).  Next to
them oracle/_ref/BUILD_INFO.json records the SHA-256 of every reference source, of the recipe and of the wrapper, and the
compiler version; ``lib()`` refuses a library whose recorded recipe or wrapper hash differs from the tree.  Nothing under
oracle/_ref/ is committed.  DGS_REFERENCE_ROOT names the reference tree (default /root/reference); where it is absent,
``build_ref`` leaves oracle/_ref/ as it is.

Front-end.  ``forward`` / ``backward`` / ``mark_visible`` take what tests/helpers.oracle_forward takes and return the
oracle's keys and array layouts, so the same checkers serve both.  Inputs travel as torch device tensors; the reference
synchronises on the null stream itself (it copies num_rendered to the host), so every call is bracketed by
torch.cuda.synchronize().  prefiltered and debug are always False (with prefiltered the reference's frustum test prints
and traps by design).  P == 0 returns before anything is touched, as the reference's torch binding does.
"""
import ctypes
import hashlib
import json
import os
import re
import shutil
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
REF_DIR = os.path.join(_HERE, "_ref")
SHIM_DIR = os.path.join(_HERE, "refshim")
WRAPPER = os.path.join(_HERE, "ref_rasterizer_wrap.cpp")
BUILD_INFO = os.path.join(REF_DIR, "BUILD_INFO.json")
RASTERIZER_SUBDIR = os.path.join("submodules", "diff-gaussian-rasterization")
UNITS = ("forward.cu", "backward.cu", "rasterizer_impl.cu")
# (pattern, replacement): the stated, mechanical transformations of the temporary copies
EDITS = ((r"<< <", "<<<"), (r">> >", ">>>"))
FLAGS = ("--offload-arch=gfx950", "-x", "hip", "-O2", "-std=c++17", "-fPIC", "-D__trap=__builtin_trap")
VARIANTS = {"f32": ("-ffp-contract=off",), "fma": ("-ffp-contract=fast",)}
MAX_JOBS = 8          # four translation units per library, two libraries


def reference_root():
    return os.environ.get("DGS_REFERENCE_ROOT", "/root/reference")


def _rasterizer_dir():
    return os.path.join(reference_root(), RASTERIZER_SUBDIR)


def reference_present():
    return os.path.isfile(os.path.join(_rasterizer_dir(), "cuda_rasterizer", "rasterizer_impl.cu"))


def lib_path(variant):
    return os.path.join(REF_DIR, f"libdgs_refkernels_{variant}.so")


def libraries_present():
    return all(os.path.isfile(lib_path(v)) for v in VARIANTS)


def available():
    """False only for a foreign checkout: no library under oracle/_ref/ AND no reference tree to build one from."""
    return libraries_present() or reference_present()


def _sha(path):
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def recipe_hash():
    """SHA-256 over what the recipe feeds the compiler besides the reference's sources and the wrapper: the edits, the
    flags of both variants, the unit list and every shim header."""
    h = hashlib.sha256(json.dumps([EDITS, FLAGS, sorted(VARIANTS.items()), UNITS], sort_keys=True).encode())
    for root, _, files in sorted(os.walk(SHIM_DIR)):
        for name in sorted(files):
            p = os.path.join(root, name)
            h.update(os.path.relpath(p, SHIM_DIR).encode())
            h.update(open(p, "rb").read())
    return h.hexdigest()


def wrapper_hash():
    return _sha(WRAPPER)


def _compiler_version(hipcc):
    out = subprocess.run([hipcc, "--version"], capture_output=True, text=True).stdout
    return " | ".join(line.strip() for line in out.splitlines() if "version" in line.lower())


def _read_info():
    try:
        with open(BUILD_INFO) as f:
            return json.load(f)
    except (OSError, ValueError):
        return None


def build_ref(force=False, verbose=False):
    """Runs the recipe.  Returns the two library paths, or None where the reference tree is absent (oracle/_ref/ is then
    left as it is).  Up to date (same sources, recipe, wrapper and compiler) means nothing is compiled."""
    if not reference_present():
        return None
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src_dir = os.path.join(_rasterizer_dir(), "cuda_rasterizer")
    names = sorted(n for n in os.listdir(src_dir) if n.endswith((".cu", ".h")))
    info = {"reference_sources": {n: _sha(os.path.join(src_dir, n)) for n in names}, "recipe": recipe_hash(),
            "wrapper": wrapper_hash(), "compiler": _compiler_version(hipcc)}
    if not force and libraries_present() and _read_info() == info:
        return [lib_path(v) for v in VARIANTS]
    os.makedirs(REF_DIR, exist_ok=True)
    tmp = tempfile.mkdtemp(prefix="dgs_refkernels_")
    try:
        copies = os.path.join(tmp, "cuda_rasterizer")
        os.makedirs(copies)
        for n in names:
            with open(os.path.join(src_dir, n), encoding="utf-8", errors="surrogateescape") as f:
                text = f.read()
            for pat, rep in EDITS:
                text = re.sub(pat, rep, text)
            with open(os.path.join(copies, n), "w", encoding="utf-8", errors="surrogateescape") as f:
                f.write(text)
        inc = ["-I" + SHIM_DIR, "-I" + copies, "-I" + os.path.join(_rasterizer_dir(), "third_party", "glm")]
        jobs = []
        for v, extra in VARIANTS.items():
            for src in [os.path.join(copies, u) for u in UNITS] + [WRAPPER]:
                obj = os.path.join(tmp, f"{v}_{os.path.basename(src)}.o")
                jobs.append((v, [hipcc, *FLAGS, *extra, *inc, "-c", src, "-o", obj], obj))

        def run(job):
            r = subprocess.run(job[1], capture_output=True, text=True)
            if r.returncode != 0:
                raise RuntimeError("reference kernels: compile failed\n" + " ".join(job[1]) + "\n" + r.stderr[-4000:])
            if verbose and r.stderr.strip():
                print(r.stderr[-2000:])

        with ThreadPoolExecutor(max_workers=min(MAX_JOBS, os.cpu_count() or 1, 16)) as pool:
            list(pool.map(run, jobs))
        for v in VARIANTS:
            objs = [j[2] for j in jobs if j[0] == v]
            out = os.path.join(tmp, os.path.basename(lib_path(v)))
            r = subprocess.run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", out, *objs],
                               capture_output=True, text=True)
            if r.returncode != 0:
                raise RuntimeError("reference kernels: link failed\n" + r.stderr[-4000:])
            os.replace(out, lib_path(v))
        with open(BUILD_INFO, "w") as f:
            json.dump(info, f, indent=1, sort_keys=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return [lib_path(v) for v in VARIANTS]


# ------------------------------------------------------------------------------------------------------ loader
class _State(ctypes.Structure):       # mirrors DgsRefState (ref_rasterizer_wrap.cpp)
    _fields_ = [("P", ctypes.c_int32), ("N", ctypes.c_int32), ("R", ctypes.c_int32), ("tiles", ctypes.c_int32)] + [
        (n, ctypes.c_void_p) for n in ("depths", "pre_sigmoid", "internal_radii", "means2D", "cov3D", "conic_opacity", "rgb",
                                       "point_offsets", "tiles_touched", "point_list_keys", "point_list", "ranges",
                                       "n_contrib", "accum_alpha")]


_libs = {}


def check_build_info():
    """Raises unless oracle/_ref/ holds both libraries and a BUILD_INFO.json whose recipe and wrapper hashes are the tree's."""
    if not libraries_present():
        raise RuntimeError("oracle/_ref/ holds no reference-kernel libraries: run __graft_entry__.build() where the "
                           "reference tree is present")
    info = _read_info()
    if info is None:
        raise RuntimeError("oracle/_ref/BUILD_INFO.json is missing or unreadable")
    if info.get("recipe") != recipe_hash() or info.get("wrapper") != wrapper_hash():
        raise RuntimeError("oracle/_ref/ was built from another recipe or wrapper than this tree's (BUILD_INFO.json): "
                           "rebuild it with __graft_entry__.build()")
    return info


def lib(variant="f32"):
    if variant not in _libs:
        if not libraries_present() and reference_present():
            build_ref()
        check_build_info()
        L = ctypes.CDLL(lib_path(variant))
        L.dgs_ref_create.restype = ctypes.c_void_p
        L.dgs_ref_destroy.argtypes = [ctypes.c_void_p]
        L.dgs_ref_last_error.restype = ctypes.c_char_p
        L.dgs_ref_state.argtypes = [ctypes.c_void_p, ctypes.POINTER(_State)]
        L.dgs_ref_copy_out.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
        assert L.dgs_ref_struct_size() == ctypes.sizeof(_State)
        _libs[variant] = L
    return _libs[variant]


class _Handle:
    def __init__(self, L):
        self.L, self.h = L, ctypes.c_void_p(L.dgs_ref_create())

    def __del__(self):
        if self.h:
            self.L.dgs_ref_destroy(self.h)
            self.h = None


def _dev(a, dtype=None):
    import torch
    if a is None:
        return None
    t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype or np.float32))
    return t.to("cuda").contiguous()


def _ptr(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _fail(L, what, rc):
    raise RuntimeError(f"reference kernels, {what}: rc {rc}: {L.dgs_ref_last_error().decode()}")


def _fetch(L, ptr, dtype, shape):
    out = np.zeros(shape, dtype)
    if out.nbytes:
        rc = L.dgs_ref_copy_out(out.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(ptr), out.nbytes)
        if rc != 0:
            _fail(L, "copy_out", rc)
    return out


def empty_forward(scene, M=0):
    """What the reference's binding returns for P == 0 (rasterize_points.cu guards on P != 0): zero images, no launch."""
    W, H = scene["W"], scene["H"]
    T = ((W + 15) // 16) * ((H + 15) // 16)
    z = lambda *s: np.zeros(s, np.float32)
    return dict(P=0, M=M, W=W, H=H, radii=np.zeros(0, np.int32), tiles_touched=np.zeros(0, np.uint32), means2D=z(0, 2),
                depths=z(0), conic_opacity=z(0, 4), rgb=z(0, 3), pre_sigmoid=z(0, 3), cov3D=z(0, 6),
                keys=np.zeros(0, np.uint64), point_list=np.zeros(0, np.uint32), ranges=np.zeros((T, 2), np.uint32),
                num_rendered=0, color=z(3, H, W), depth=z(1, H, W), n_contrib=np.zeros(W * H, np.uint32), final_T=z(W * H))


def forward(scene, k, sh_degree=None, use_sigmoid=False, colors_precomp=None, cov3D_precomp=None, scale_modifier=1.0,
            variant="f32"):
    """The reference's forward for subframe k of `scene`; the arguments of tests/helpers.oracle_forward.  Returns the
    oracle's keys, copied out of the reference's Geometry / Binning / Image state."""
    import torch
    P, W, H = int(np.asarray(scene["means3D"]).reshape(-1, 3).shape[0]), scene["W"], scene["H"]
    D = int(scene["sh_degree"] if sh_degree is None else sh_degree)
    sh = None if colors_precomp is not None else np.asarray(scene["sh"], np.float32)
    M = 0 if sh is None else int(sh.shape[1])
    if P == 0:
        return empty_forward(scene, M)
    L = lib(variant)
    t = dict(means3D=_dev(np.asarray(scene["means3D"]).reshape(-1, 3)), sh=_dev(sh), colors_precomp=_dev(colors_precomp),
             opacities=_dev(np.asarray(scene["opacities"]).reshape(-1)),
             scales=None if cov3D_precomp is not None else _dev(scene["scales"]),
             rotations=None if cov3D_precomp is not None else _dev(scene["rotations"]), cov3D_precomp=_dev(cov3D_precomp),
             viewmatrix=_dev(np.asarray(scene["viewmatrix"][k]).reshape(16)),
             projmatrix=_dev(np.asarray(scene["projmatrix"][k]).reshape(16)),
             campos=_dev(np.asarray(scene["campos"][k]).reshape(3)), bg=_dev(np.asarray(scene["bg"]).reshape(3)))
    color = torch.zeros((3, H, W), device="cuda")
    depth = torch.zeros((1, H, W), device="cuda")
    radii = torch.zeros(P, dtype=torch.int32, device="cuda")
    par = dict(P=P, D=D, M=M, W=W, H=H, tanfovx=float(scene["tanfovx"]), tanfovy=float(scene["tanfovy"]),
               z_near=float(scene["z_near"]), z_far=float(scene["z_far"]), scale_modifier=float(scale_modifier),
               use_sigmoid=int(bool(use_sigmoid)))
    hd = _Handle(L)
    f = ctypes.c_float
    torch.cuda.synchronize()
    R = L.dgs_ref_forward(hd.h, P, D, M, _ptr(t["bg"]), W, H, _ptr(t["means3D"]), _ptr(t["sh"]), _ptr(t["colors_precomp"]),
                          _ptr(t["opacities"]), _ptr(t["scales"]), f(par["scale_modifier"]), _ptr(t["rotations"]),
                          _ptr(t["cov3D_precomp"]), _ptr(t["viewmatrix"]), _ptr(t["projmatrix"]), _ptr(t["campos"]),
                          f(par["tanfovx"]), f(par["tanfovy"]), f(par["z_near"]), f(par["z_far"]), _ptr(color), _ptr(depth),
                          _ptr(radii), par["use_sigmoid"])
    torch.cuda.synchronize()
    if R < 0:
        _fail(L, "forward", R)
    s = _State()
    rc = L.dgs_ref_state(hd.h, ctypes.byref(s))
    if rc != 0:
        _fail(L, "state", rc)
    assert (s.P, s.N, s.R) == (P, W * H, R)
    N, T = W * H, s.tiles
    st = dict(P=P, M=M, D=D, W=W, H=H, num_rendered=int(R), radii=radii.cpu().numpy(),
              color=color.cpu().numpy(), depth=depth.cpu().numpy(),
              depths=_fetch(L, s.depths, np.float32, (P,)), pre_sigmoid=_fetch(L, s.pre_sigmoid, np.float32, (P, 3)),
              internal_radii=_fetch(L, s.internal_radii, np.int32, (P,)), means2D=_fetch(L, s.means2D, np.float32, (P, 2)),
              cov3D=_fetch(L, s.cov3D, np.float32, (P, 6)), conic_opacity=_fetch(L, s.conic_opacity, np.float32, (P, 4)),
              rgb=_fetch(L, s.rgb, np.float32, (P, 3)),
              point_offsets_inclusive=_fetch(L, s.point_offsets, np.uint32, (P,)),
              tiles_touched=_fetch(L, s.tiles_touched, np.uint32, (P,)),
              keys=_fetch(L, s.point_list_keys, np.uint64, (R,)), point_list=_fetch(L, s.point_list, np.uint32, (R,)),
              ranges=_fetch(L, s.ranges, np.uint32, (T, 2)), n_contrib=_fetch(L, s.n_contrib, np.uint32, (N,)),
              final_T=_fetch(L, s.accum_alpha, np.float32, (N,)))
    st["_ctx"] = dict(L=L, handle=hd, t=t, par=par, radii=radii)
    return st


def backward(st, dL_dcolor, dL_ddepth=None):
    """The reference's backward of the forward that produced `st`.  Returns the oracle's gradient keys (oracle.backward)."""
    import torch
    c = st["_ctx"]
    L, t, par, hd = c["L"], c["t"], c["par"], c["handle"]
    P, M, W, H = par["P"], par["M"], par["W"], par["H"]
    gC = _dev(np.asarray(dL_dcolor, np.float32).reshape(3, H, W))
    gD = torch.zeros((1, H, W), device="cuda") if dL_ddepth is None else _dev(np.asarray(dL_ddepth, np.float32).reshape(1, H, W))
    z = lambda *s: torch.zeros(s, device="cuda")
    g = dict(dL_dmeans2D=z(P, 3), dL_dconic=z(P, 4), dL_dopacity=z(P, 1), dL_dcolors=z(P, 3), dL_dmeans3D=z(P, 3),
             dL_dcov3D=z(P, 6), dL_dsh=z(P, max(M, 1), 3), dL_dscales=z(P, 3), dL_drotations=z(P, 4), dL_ddepths=z(P, 1),
             dL_dviewmatrix=z(4, 4), dL_dprojmatrix=z(4, 4))
    f = ctypes.c_float
    torch.cuda.synchronize()
    rc = L.dgs_ref_backward(hd.h, P, par["D"], M, _ptr(t["bg"]), W, H, _ptr(t["means3D"]), _ptr(t["sh"]),
                            _ptr(t["colors_precomp"]), _ptr(t["scales"]), f(par["scale_modifier"]), _ptr(t["rotations"]),
                            _ptr(t["cov3D_precomp"]), _ptr(t["viewmatrix"]), _ptr(t["projmatrix"]), _ptr(t["campos"]),
                            f(par["tanfovx"]), f(par["tanfovy"]), f(par["z_near"]), f(par["z_far"]), _ptr(c["radii"]),
                            _ptr(gC), _ptr(gD), _ptr(g["dL_dmeans2D"]), _ptr(g["dL_dconic"]), _ptr(g["dL_dopacity"]),
                            _ptr(g["dL_dcolors"]), _ptr(g["dL_dmeans3D"]), _ptr(g["dL_dcov3D"]), _ptr(g["dL_dsh"]),
                            _ptr(g["dL_dscales"]), _ptr(g["dL_drotations"]), _ptr(g["dL_ddepths"]), _ptr(g["dL_dviewmatrix"]),
                            _ptr(g["dL_dprojmatrix"]), par["use_sigmoid"])
    torch.cuda.synchronize()
    if rc != 0:
        _fail(L, "backward", rc)
    out = {name: v.cpu().numpy() for name, v in g.items()}
    out["dL_dsh"] = out["dL_dsh"][:, :M]
    return out


def forward_backward(scene, K, dL_dcolor, dL_ddepth=None, variant="f32", states=None, **kw):
    """K calls (the reference has no fused call) in the shape tests/helpers.assert_grads_close takes on the product's side:
    per-Gaussian gradients summed over k as autograd does in the reference's loop, per-subframe ones stacked.  states: the
    forwards of an earlier call, to run the backward alone again (the atomics' order differs from run to run)."""
    sts = states if states is not None else [forward(scene, k, variant=variant, **kw) for k in range(K)]
    gs = [backward(sts[k], dL_dcolor[k], None if dL_ddepth is None else dL_ddepth[k]) for k in range(K)]
    r = {}
    for name, key in (("dL_dmeans3D", "dL_dmeans3D"), ("dL_dopacities", "dL_dopacity"), ("dL_dsh", "dL_dsh"),
                      ("dL_dscales", "dL_dscales"), ("dL_drotations", "dL_drotations"), ("dL_dcolors_precomp", "dL_dcolors"),
                      ("dL_dcov3D_precomp", "dL_dcov3D"), ("dL_dcov3D", "dL_dcov3D")):
        r[name] = sum(g[key].astype(np.float64) for g in gs)
    for name in ("dL_dmeans2D", "dL_dviewmatrix", "dL_dprojmatrix"):
        r[name] = np.stack([g[name] for g in gs]).astype(np.float64)
    r["dL_dconic"] = np.stack([g["dL_dconic"][:, [0, 1, 3]] for g in gs]).astype(np.float64)
    r["states"] = sts
    return r


def mark_visible(means3D, viewmatrix, projmatrix, variant="f32"):
    import torch
    m = _dev(np.asarray(means3D, np.float32).reshape(-1, 3))
    P = m.shape[0]
    if P == 0:
        return np.zeros(0, bool)
    L = lib(variant)
    present = torch.zeros(P, dtype=torch.bool, device="cuda")
    v, p = _dev(np.asarray(viewmatrix).reshape(16)), _dev(np.asarray(projmatrix).reshape(16))
    torch.cuda.synchronize()
    rc = L.dgs_ref_mark_visible(P, _ptr(m), _ptr(v), _ptr(p), _ptr(present))
    torch.cuda.synchronize()
    if rc != 0:
        _fail(L, "mark_visible", rc)
    return present.cpu().numpy()
