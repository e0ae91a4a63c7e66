"""ctypes binding of libeonerf_hip.so (the headers of include/): one table of the C ABI, the build, the load.

PyTorch is plumbing here: it owns device memory (tensor.data_ptr()) and the current HIP stream; every arithmetic
step of the hot path runs inside the HIP library.  There is NO fallback: if the library is missing, cannot be
loaded, or no GPU is present, the product path raises.
"""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIB_PATH = os.environ.get("EONERF_LIB") or os.path.join(CSRC, "libeonerf_hip.so")   # EONERF_LIB: A/B builds of the same ABI

EONERF_FP32, EONERF_BF16, EONERF_F16X3 = 0, 1, 2
PRECISIONS = {"fp32": EONERF_FP32, "bf16": EONERF_BF16, "fp16x3": EONERF_F16X3}
F_SHADOWS, F_EVAL, F_TRAIN, F_ONLY_DEPTH, F_RGB_LOSS = 1, 2, 4, 8, 16


class EonerfRpc(C.Structure):
    _fields_ = [("col_num", C.c_double * 20), ("col_den", C.c_double * 20), ("row_num", C.c_double * 20), ("row_den", C.c_double * 20),
                ("row_offset", C.c_double), ("col_offset", C.c_double), ("lat_offset", C.c_double), ("lon_offset", C.c_double),
                ("alt_offset", C.c_double), ("row_scale", C.c_double), ("col_scale", C.c_double), ("lat_scale", C.c_double),
                ("lon_scale", C.c_double), ("alt_scale", C.c_double)]


class EonerfConfig(C.Structure):
    _fields_ = [("n_images", C.c_int), ("precision", C.c_int), ("n_samples", C.c_int), ("radiometric", C.c_int)]


# The whole C ABI: public header -> entry point -> (return type, argument types), one line per prototype.  lib() binds exactly this,
# build() digests exactly these headers, and tests/test_library_abi.py holds every line against the header's prototype.
vp, cp, i, lg, sz, fp, d = C.c_void_p, C.c_char_p, C.c_int, C.c_long, C.c_size_t, C.c_float, C.c_double
i64, u32, u64 = C.c_int64, C.c_uint32, C.c_uint64
f3, d3, rpc = C.POINTER(fp), C.POINTER(d), C.POINTER(EonerfRpc)
API = {
    # the context and the training / rendering entry points (radiance_fields/eonerf.py, trainer.py, sat_rendering.py, datasets/satellite.py)
    "eonerf_hip.h": {
        "eonerf_version": (i, []),
        "eonerf_strerror": (cp, [i]),
        "eonerf_create": (i, [C.POINTER(vp), C.POINTER(EonerfConfig)]),
        "eonerf_destroy": (i, [vp]),
        "eonerf_param_tensors": (i, [vp]),
        "eonerf_param_info": (i, [vp, i, C.POINTER(cp), C.POINTER(sz), C.POINTER(i), C.POINTER(i)]),
        "eonerf_param_floats": (sz, [vp]),
        "eonerf_set_weights": (i, [vp, vp, vp]),
        "eonerf_field_workspace_bytes": (sz, [vp, i]),
        "eonerf_render_workspace_bytes": (sz, [vp, i, i]),
        "eonerf_field_forward": (i, [vp, vp, vp, vp, vp, i, vp, vp, vp, vp, vp, vp, sz, vp]),
        "eonerf_query_density": (i, [vp, vp, vp, i, vp, vp, sz, vp]),
        "eonerf_render_forward": (i, [vp, vp, vp, vp, vp, vp, vp, vp, i, i, vp, vp, vp, sz, vp]),
        "eonerf_render_backward": (i, [vp, vp, vp, vp, i, i, vp, vp, vp, sz, vp]),
        "eonerf_adam_step": (i, [vp, vp, vp, vp, vp, i, fp, fp, fp, fp, fp, vp, vp]),
        "eonerf_profile_enable": (i, [vp, i]),
        "eonerf_profile_read": (i, [vp, i, f3, C.POINTER(i)]),
        "eonerf_train_loss": (i, [vp, vp, vp, i, i, vp, vp, vp]),
        "eonerf_sample_rays": (i, [vp, vp, vp, vp, i, i, vp, vp, vp, vp, vp, vp, sz, vp]),
        "eonerf_rendering": (i, [vp, vp, vp, vp, vp, vp, vp, i, i, i, vp, vp, vp, vp, vp, vp, vp, sz, vp]),
        "eonerf_generate_rays": (i, [rpc, vp, vp, lg, i, d, d, i, i, d, d, f3, f3, vp, vp, vp, vp]),
        "eonerf_field_train_workspace_bytes": (sz, [vp, i, i]),
        "eonerf_field_forward_train": (i, [vp, vp, vp, vp, vp, i, i, vp, vp, vp, vp, vp, vp, sz, vp]),
        "eonerf_field_backward": (i, [vp, vp, vp, i, i, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]),
        "eonerf_set_noise_seed": (i, [vp, u64]),
        "eonerf_render_status": (i, [vp, i, i, vp, sz, vp]),
        "eonerf_device_status": (i, [vp, vp]),
        "eonerf_grad_floats": (sz, [vp]),
        "eonerf_grad_seal": (i, [vp, vp, vp]),
        "eonerf_profile_name": (cp, [i]),
        "eonerf_adam_step_zero_grad": (i, [vp, vp, vp, vp, vp, i, fp, fp, fp, fp, fp, vp, vp]),
        "eonerf_rendering_train": (i, [vp, vp, vp, vp, vp, vp, vp, i, i, i, vp, vp, vp, vp, vp, vp, vp, sz, vp]),
        "eonerf_rendering_backward": (i, [vp, vp, vp, vp, i, i, vp, vp, vp, vp, vp, vp, vp, sz, vp]),
        "eonerf_clock_probe": (i, [vp, vp, vp]),
        "eonerf_range_status": (i, [vp, vp]),
        "eonerf_set_n_samples": (i, [vp, i]),
        "eonerf_render_backward_loss": (i, [vp, vp, vp, vp, i, i, vp, vp, i, vp, vp, vp, vp, sz, vp]),
        "eonerf_presample": (i, [vp, vp, vp, vp, i, i, vp, vp, sz, vp]),
        "eonerf_presample_cancel": (i, [vp]),
        "eonerf_grad_early_floats": (sz, [vp]),
        "eonerf_set_exchange_event": (i, [vp, vp, i]),
    },
    # the stateless DSM evaluation group of the same library (dsm.py)
    "eonerf_dsm.h": {
        "eonerf_dsm_version": (i, []),
        "eonerf_nadir_rays": (i, [i, i, d, d, d, d, d, d3, d, d, vp, vp]),
        "eonerf_dsm_rasterize": (i, [vp, i, vp, lg, d3, d3, d, d, i, i, d, vp, vp, vp, vp]),
        "eonerf_dsm_mask_water": (i, [vp, i, i, vp, i, i, vp]),
        "eonerf_dsm_register_workspace_bytes": (sz, [i, i, i, i]),
        "eonerf_dsm_register_levels": (i, [i, i]),
        "eonerf_dsm_register_level": (i, [i, i, i, i, i, C.POINTER(i), C.POINTER(sz)]),
        "eonerf_dsm_register": (i, [vp, i, i, vp, i, i, i, vp, vp, sz, vp]),
        "eonerf_dsm_mae_workspace_bytes": (sz, []),
        "eonerf_dsm_mae": (i, [vp, i, i, vp, i, i, vp, i, i, vp, vp, vp, vp, sz, vp]),
    },
    # the stateless depth-prior group (priors.py): initial DSM -> per-ray depth / confidence
    "eonerf_prior.h": {
        "eonerf_prior_version": (i, []),
        "eonerf_prior_workspace_bytes": (sz, [i, i]),
        "eonerf_prior_reproject": (i, [vp, vp, i, i, d3, rpc, i, i, i, i, vp, i, vp, i, fp, fp, vp, vp, sz, vp]),
    },
    # the stateless per-image validation metrics (validation.py): uncertainty loss, MSE, PSNR
    "eonerf_metrics.h": {
        "eonerf_metrics_version": (i, []),
        "eonerf_metrics_workspace_bytes": (sz, []),
        "eonerf_image_metrics": (i, [vp, i, vp, i, vp, i, lg, vp, vp, sz, vp]),
    },
    # one view under K sun directions from one camera pass (relight.py)
    "eonerf_sweep.h": {
        "eonerf_sweep_version": (i, []),
        "eonerf_sun_sweep_workspace_bytes": (sz, [vp, i, i]),
        "eonerf_render_sun_sweep": (i, [vp, vp, vp, vp, vp, vp, vp, vp, vp, i, i, i, vp, vp, vp, sz, vp]),
    },
    # the occupancy grid (occupancy.py): update, dilation, the grid of a context's export renders, the pinned sampler
    "eonerf_occ.h": {
        "eonerf_occ_version": (i, []),
        "eonerf_occ_workspace_bytes": (sz, [vp, i]),
        "eonerf_occ_update": (i, [vp, vp, vp, vp, i, fp, fp, fp, i, u32, vp, vp, vp, sz, vp]),
        "eonerf_occ_dilate": (i, [vp, vp, i, vp]),
        "eonerf_set_occupancy": (i, [vp, vp, i]),
        "eonerf_occ_sample_rays": (i, [vp, vp, vp, vp, i, i, vp, i, vp, vp, vp, vp, vp, vp, sz, vp]),
    },
    # block-wise early ray termination of export renders (sat_rendering.render_image(early_stop_eps=...))
    "eonerf_march.h": {
        "eonerf_march_version": (i, []),
        "eonerf_march_workspace_bytes": (sz, [vp, i, i, i]),
        "eonerf_render_forward_march": (i, [vp, vp, vp, vp, vp, vp, vp, vp, i, i, fp, i, vp, vp, vp, vp, sz, vp]),
        "eonerf_march_sample_round": (i, [vp, vp, vp, vp, i, i, i, i, vp, vp, vp, vp, vp, vp, sz, vp]),
    },
    # quantile depth of export renders (sat_rendering.render_depth_quantiles)
    "eonerf_quantile.h": {
        "eonerf_quantile_version": (i, []),
        "eonerf_quantile_workspace_bytes": (sz, [vp, i, i, i]),
        "eonerf_render_depth_quantiles": (i, [vp, vp, vp, vp, vp, vp, i, vp, i, fp, i, vp, vp, vp, vp, vp, vp, vp, sz, vp]),
    },
    # the stateless true-orthophoto group (ortho.py): surface points, per-image gather, fusion
    "eonerf_ortho.h": {
        "eonerf_ortho_version": (i, []),
        "eonerf_ortho_ground": (i, [vp, i, vp, lg, f3, f3, i, i, vp, vp]),
        "eonerf_ortho_gather": (i, [vp, lg, rpc, vp, i, i, i, f3, f3, vp, fp, vp, vp, vp, vp]),
        "eonerf_ortho_fuse": (i, [vp, vp, i, lg, i, i, vp, vp, vp, vp]),
    },
    # camera offset refinement (pose.py): the ray-origin gradient behind a render backward and its per-image sum
    "eonerf_pose.h": {
        "eonerf_pose_version": (i, []),
        "eonerf_origin_grad_scratch_bytes": (sz, [vp, i, i]),
        "eonerf_render_origin_grad": (i, [vp, vp, vp, vp, i, i, vp, sz, vp, sz, vp, vp, vp]),
    },
    # the forward-mode density gradient and the surface normals of export renders (normals.py)
    "eonerf_normals.h": {
        "eonerf_normals_version": (i, []),
        "eonerf_density_grad_workspace_bytes": (sz, [vp, i]),
        "eonerf_field_density_grad": (i, [vp, vp, vp, i, vp, vp, vp, sz, vp]),
        "eonerf_normals_workspace_bytes": (sz, [vp, i]),
        "eonerf_render_normals": (i, [vp, vp, vp, vp, vp, vp, i, f3, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]),
    },
    # the stateless mesh export group (mesh.py): marching tetrahedra over a sampled density volume
    "eonerf_mesh.h": {
        "eonerf_mesh_version": (i, []),
        "eonerf_mesh_lattice_points": (i, [f3, f3, i, i, i, i, vp, vp]),
        "eonerf_mesh_workspace_bytes": (sz, [i, i, i]),
        "eonerf_mesh_count": (i, [vp, i, i, i, fp, vp, vp, sz, vp]),
        "eonerf_mesh_emit": (i, [vp, i, i, i, fp, f3, f3, vp, sz, vp, i64, vp, i64, vp, vp, vp]),
    },
    # connected components of a volume under the mesher's connectivity, and the floater / cavity filter (mesh.py)
    "eonerf_components.h": {
        "eonerf_cc_version": (i, []),
        "eonerf_cc_workspace_bytes": (sz, [i, i, i]),
        "eonerf_cc_label": (i, [vp, i, i, i, fp, i, vp, vp, vp, vp, sz, vp]),
        "eonerf_cc_filter": (i, [vp, vp, vp, i, i, i, i, i64, i, vp, vp, vp]),
    },
    # a mesh rasterised from above into a DSM, a face raster and attribute rasters (mesh.rasterize_mesh)
    "eonerf_mesh_dsm.h": {
        "eonerf_mesh_dsm_version": (i, []),
        "eonerf_mesh_dsm_rasterize": (i, [vp, i64, vp, i64, d3, d3, d, d, i, i, d, vp, vp, vp, vp, vp]),
        "eonerf_mesh_dsm_attributes": (i, [vp, i64, vp, i64, d3, d3, d, d, i, i, d, vp, vp, i, vp, vp]),
    },
    # the read-only workspace layout query (tests decode the saved slabs through it)
    "eonerf_layout.h": {
        "eonerf_layout_version": (i, []),
        "eonerf_workspace_layout": (i, [vp, i, i, i, C.POINTER(u64), i]),
        "eonerf_ray_layout": (i, [vp, i, i, C.POINTER(u64), i]),
    },
}

# Staged groups: their headers lie in csrc/ (build() digests every header there) until a follow-up moves them into include/ and their
# tables into API.  lib() binds them after API; tests/test_simplify_abi_cpu.py holds every line against the header's prototype.
i3 = C.POINTER(i)
API_STAGED = {
    # mesh simplification by vertex clustering (mesh.simplify_mesh)
    "eonerf_simplify.h": {
        "eonerf_simplify_version": (i, []),
        "eonerf_simplify_workspace_bytes": (sz, [i3, i64, i64]),
        "eonerf_simplify_count": (i, [vp, i64, vp, i64, f3, f3, i3, vp, sz, vp, vp]),
        "eonerf_simplify_emit": (i, [vp, i64, vp, i64, f3, f3, i3, i, vp, sz, vp, i64, vp, i64, vp, vp, vp, vp]),
    },
}
# A table of its own (tests/test_simplify_abi_cpu.py pins the set of headers in API_STAGED); tests/test_smooth_abi_cpu.py holds it to
# the header.  lib() binds it after API_STAGED.
i32p = C.POINTER(C.c_int32)
API_STAGED_SMOOTH = {
    # Taubin lambda|mu smoothing in fixed point (mesh.smooth_mesh)
    "eonerf_smooth.h": {
        "eonerf_smooth_version": (i, []),
        "eonerf_smooth_workspace_bytes": (sz, [i64, i64]),
        "eonerf_smooth_build": (i, [vp, i64, vp, i64, f3, f3, vp, i, vp, sz, vp, vp]),
        "eonerf_smooth_run": (i, [vp, i64, i64, f3, f3, i32p, i, vp, sz, vp, vp, vp]),
    },
}
# Likewise a table of its own (the two staged ABI tests pin the tables above); tests/test_raycast_abi_cpu.py holds it to the header.
# lib() binds it after API_STAGED_SMOOTH.
API_STAGED_RAYCAST = {
    # rays against a mesh through a uniform grid (mesh.MeshRaycaster, mesh.render_mesh, mesh.vertex_visibility)
    "eonerf_raycast.h": {
        "eonerf_raycast_version": (i, []),
        "eonerf_raycast_workspace_bytes": (sz, [i3, i64, i64]),
        "eonerf_raycast_count": (i, [vp, i64, vp, i64, d3, d3, i3, vp, vp, vp]),
        "eonerf_raycast_build": (i, [vp, i64, vp, i64, d3, d3, i3, vp, i64, vp, sz, vp]),
        "eonerf_raycast_closest": (i, [vp, i64, vp, i64, d3, d3, i3, i64, vp, sz, vp, i64, vp, i64, i64, d, d, vp, vp, vp, vp, vp]),
        "eonerf_raycast_occluded": (i, [vp, i64, vp, i64, d3, d3, i3, i64, vp, sz, vp, i64, vp, i64, i64, d, d, vp, vp, vp, vp]),
    },
}

# And a fourth (the three staged ABI tests pin the tables above); tests/test_texture_abi_cpu.py holds it to the header.  lib() binds it
# after API_STAGED_RAYCAST.
i64p = C.POINTER(i64)
API_STAGED_TEXTURE = {
    # the texture atlas of a mesh and the fused per-texel gather of the input images (texture.py)
    "eonerf_texture.h": {
        "eonerf_texture_version": (i, []),
        "eonerf_texture_layout": (i, [i64, i, i64p]),
        "eonerf_texture_uv": (i, [i64, i, vp, vp]),
        "eonerf_texture_samples": (i, [vp, i64, vp, i64, i, i64, i64, f3, f3, i, i, vp, vp, vp, vp, vp, vp]),
        "eonerf_texture_bake": (i, [vp, vp, i64, vp, vp, vp, i, i, vp, vp, vp, vp, fp, i, i, vp, vp, vp, vp, vp]),
    },
}

# And a fifth (the four staged ABI tests pin the tables above); tests/test_dual_abi_cpu.py holds it to the header.  lib() binds it after
# API_STAGED_TEXTURE.
API_STAGED_DUAL = {
    # dual contouring of a volume from Hermite data (mesh.dual_contour, mesh.extract_mesh(method="dual"))
    "eonerf_dual.h": {
        "eonerf_dual_version": (i, []),
        "eonerf_dual_workspace_bytes": (sz, [i, i, i]),
        "eonerf_dual_count": (i, [vp, i, i, i, fp, vp, vp, sz, vp]),
        "eonerf_dual_hermite": (i, [vp, i, i, i, fp, f3, f3, vp, sz, vp, i64, vp, vp, vp]),
        "eonerf_dual_emit": (i, [vp, i, i, i, fp, f3, f3, vp, i64, fp, vp, sz, vp, i64, vp, vp, i64, vp, vp, vp]),
    },
}


def build(verbose=False):
    """Compile libeonerf_hip.so in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    # up to date?  Decided by CONTENT (a digest of every source, kept beside the library), not by time stamps: a snapshot copied to the
    # GPU box may carry arbitrary mtimes, and the object files do not travel -- a current library must never be rebuilt there
    import hashlib
    srcs = sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".cpp", ".h")) or f == "Makefile")
    srcs += [os.path.join(_HERE, "..", "include", header) for header in API]
    h = hashlib.sha1()
    for f in srcs:
        with open(f, "rb") as fh:
            h.update(os.path.basename(f).encode() + b"\0" + fh.read())
    digest, stamp = h.hexdigest(), os.path.join(CSRC, "libeonerf_hip.digest")

    def so_digest():
        with open(LIB_PATH, "rb") as fh:
            return hashlib.sha1(fh.read()).hexdigest()

    # the stamp names the sources AND the library build() itself produced from them with the Makefile's own flags: a library that was
    # rebuilt by hand afterwards (a diagnostic build: make CXXFLAGS=... -DEO_STAMP) does not match it and is rebuilt from scratch
    recorded = open(stamp).read().split() if os.path.exists(stamp) else []
    if not os.environ.get("EONERF_LIB") and os.path.exists(LIB_PATH) and len(recorded) == 2 and recorded[0] == digest:
        if recorded[1] == so_digest():
            return LIB_PATH
        subprocess.run(["make", "-C", CSRC, "clean"], capture_output=True, text=True)
    cmd = ["make", "-C", CSRC, "-j", str(min(8, os.cpu_count() or 1))]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if verbose or r.returncode:
        print(r.stdout[-4000:])
        print(r.stderr[-8000:])
    if r.returncode:
        raise RuntimeError("building libeonerf_hip.so failed")
    if not os.environ.get("EONERF_LIB"):
        with open(stamp, "w") as fh:
            fh.write(digest + " " + so_digest() + "\n")
    return LIB_PATH


_lib = None


def lib():
    """Load the library (building it is an explicit step: __graft_entry__.build() / eonerf_code_amd._lib.build())."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(the EO-NeRF hot path has no non-HIP fallback)")
    L = C.CDLL(LIB_PATH)
    for group in (list(API.values()) + list(API_STAGED.values()) + list(API_STAGED_SMOOTH.values()) + list(API_STAGED_RAYCAST.values())
                  + list(API_STAGED_TEXTURE.values()) + list(API_STAGED_DUAL.values())):
        for name, (restype, argtypes) in group.items():
            fn = getattr(L, name)               # resolves the symbol: a missing one fails here, at load
            fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L


E_RANGE = -6


def check(rc):
    if rc != 0:
        raise RuntimeError(f"libeonerf_hip: {lib().eonerf_strerror(rc).decode()} (code {rc})")


def _ptr(t):
    """The device address of a tensor as the void* the entry points take (None: NULL)."""
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream():
    """PyTorch's current HIP stream as the hipStream_t the entry points take."""
    import torch                                # lazily: CPU tests import this module without touching torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def param_layout(ctx):
    """[(name, offset, rows, cols)] of the flat fp32 parameter buffer."""
    L = lib()
    out = []
    for k in range(L.eonerf_param_tensors(ctx)):
        name, off, r, c = C.c_char_p(), C.c_size_t(), C.c_int(), C.c_int()
        check(L.eonerf_param_info(ctx, k, C.byref(name), C.byref(off), C.byref(r), C.byref(c)))
        out.append((name.value.decode(), off.value, r.value, c.value))
    return out
