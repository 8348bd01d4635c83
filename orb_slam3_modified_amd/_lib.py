"""ctypes loader for liborbx.so (the C-ABI drop-in boundary, include/orbx.h).

The shared library is built in-tree by `python -m orb_slam3_modified_amd.build` (hipcc, gfx950).
There is no Python/CPU fallback: if the library is missing the import of any compute class raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ORBX_LIB", os.path.join(_HERE, "liborbx.so"))   # ORBX_LIB: experiment builds (tools/)
DEBUG_LIB_PATH = os.path.join(os.path.dirname(LIB_PATH), "liborbx_debug.so")   # the diagnostic ABI (include/orbx_debug.h): tests and tools only
TRAIN_LIB_PATH = os.path.join(os.path.dirname(LIB_PATH), "liborbx_train.so")   # vocabulary training (include/orbx_train.h)
STEREO_LIB_PATH = os.path.join(os.path.dirname(LIB_PATH), "liborbx_stereo.so")   # the batched stereo front-end (include/orbx_stereo.h)
BOW_LIB_PATH = os.path.join(os.path.dirname(LIB_PATH), "liborbx_bow.so")         # the batched bag of words (include/orbx_bow.h)
MATCH_LIB_PATH = os.path.join(os.path.dirname(LIB_PATH), "liborbx_match.so")     # the batched SearchByBoW (include/orbx_match.h)
INITMATCH_LIB_PATH = os.path.join(os.path.dirname(LIB_PATH), "liborbx_initmatch.so")   # the batched SearchForInitialization (include/orbx_initmatch.h)
TRIMATCH_LIB_PATH = os.path.join(os.path.dirname(LIB_PATH), "liborbx_trimatch.so")     # the batched SearchForTriangulation (include/orbx_trimatch.h)
FUSE_LIB_PATH = os.path.join(os.path.dirname(LIB_PATH), "liborbx_fuse.so")             # the batched Fuse search (include/orbx_fuse.h)
MPDESC_LIB_PATH = os.path.join(os.path.dirname(LIB_PATH), "liborbx_mpdesc.so")         # the batched ComputeDistinctiveDescriptors (include/orbx_mpdesc.h)
SCORE_LIB_PATH = os.path.join(os.path.dirname(LIB_PATH), "liborbx_score.so")           # the six DBoW2 scorings (include/orbx_score.h)
FISHEYE_LIB_PATH = os.path.join(os.path.dirname(LIB_PATH), "liborbx_fisheye.so")       # the batched two-camera rig front-end (include/orbx_fisheye.h)
LOCALMATCH_LIB_PATH = os.path.join(os.path.dirname(LIB_PATH), "liborbx_localmatch.so")   # the batched SearchLocalPoints (include/orbx_localmatch.h)
LASTMATCH_LIB_PATH = os.path.join(os.path.dirname(LIB_PATH), "liborbx_lastmatch.so")     # the batched SearchByProjection(Frame, LastFrame) (include/orbx_lastmatch.h)
PROJMATCH_LIB_PATH = os.path.join(os.path.dirname(LIB_PATH), "liborbx_projmatch.so")     # the batched relocalization and Sim3 SearchByProjection (include/orbx_projmatch.h)

PLACE_LIB_PATH = os.path.join(os.path.dirname(LIB_PATH), "liborbx_place.so")             # the batched place recognition (include/orbx_place.h)
PLACEINDEX_LIB_PATH = os.path.join(os.path.dirname(LIB_PATH), "liborbx_placeindex.so")   # the same through a device inverted file (include/orbx_placeindex.h)
FRUSTUM_LIB_PATH = os.path.join(os.path.dirname(LIB_PATH), "liborbx_frustum.so")         # the batched Frame::isInFrustum (include/orbx_frustum.h)
PROJECT_LIB_PATH = os.path.join(os.path.dirname(LIB_PATH), "liborbx_project.so")         # the LastFrame, relocalization and Fuse projections (include/orbx_project.h)
SIM3_LIB_PATH = os.path.join(os.path.dirname(LIB_PATH), "liborbx_sim3.so")               # LoopClosing's Sim3 projections and agreement pass (include/orbx_sim3.h)
RIGMATCH_LIB_PATH = os.path.join(os.path.dirname(LIB_PATH), "liborbx_rigmatch.so")       # the two-camera rig blocks of the two Tracking matchers (include/orbx_rigmatch.h)
RIGBOW_LIB_PATH = os.path.join(os.path.dirname(LIB_PATH), "liborbx_rigbow.so")           # the rig block of SearchByBoW and the stacked rig frame (include/orbx_rigbow.h)
MPGEOM_LIB_PATH = os.path.join(os.path.dirname(LIB_PATH), "liborbx_mpgeom.so")           # the batched MapPoint::UpdateNormalAndDepth (include/orbx_mpgeom.h)

ORBX_OK, ORBX_E_INVALID, ORBX_E_EMPTY, ORBX_E_DEVICE, ORBX_E_CAPACITY, ORBX_E_FORMAT = 0, -1, -2, -3, -4, -5
NUM_KERNELS = 6

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"),
                     ("octave", "<i4"), ("class_id", "<i4")])
assert KP_DTYPE.itemsize == 28


class OrbxError(RuntimeError):
    def __init__(self, code: int, msg: str = ""):
        super().__init__(f"orbx error {code}: {msg}")
        self.code = code


_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} not built — run `python -m orb_slam3_modified_amd.build` "
                          "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    L = C.CDLL(LIB_PATH)
    vp, i32, sz, f32 = C.c_void_p, C.c_int, C.c_size_t, C.c_float
    ip = C.POINTER(C.c_int)
    sig = {
        "orbx_create": (i32, [C.POINTER(vp), i32, f32, i32, i32, i32, i32]),
        "orbx_destroy": (None, [vp]),
        "orbx_last_error": (C.c_char_p, [vp]),
        "orbx_keypoint_capacity": (i32, [vp]),
        "orbx_levels": (i32, [vp]),
        "orbx_scale_tables": (i32, [vp, vp, vp, vp, vp, vp]),
        "orbx_extract": (i32, [vp, vp, i32, i32, sz, i32, i32, vp, vp, ip, ip]),
        "orbx_extract_color": (i32, [vp, vp, i32, i32, C.c_size_t, i32, i32, i32, i32, vp, vp, ip, ip]),
        "orbx_extract_resized": (i32, [vp, vp, i32, i32, sz, i32, i32, i32, i32, vp, vp, ip, ip]),
        "orbx_extract_batch_device": (i32, [vp, vp, i32, i32, i32, sz, sz, i32, i32, vp, vp, vp, vp]),
        "orbx_extract_batch": (i32, [vp, vp, i32, i32, i32, sz, sz, i32, i32, vp, vp, vp]),
        "orbx_pyramid_level": (i32, [vp, i32, i32, vp, sz, ip, ip]),
        "orbx_set_host_pyramid": (i32, [vp, i32]),
        "orbx_host_pyramid_level": (i32, [vp, i32, C.POINTER(vp), C.POINTER(sz), ip, ip]),
        "orbx_profile_enable": (i32, [vp, i32]),
        "orbx_profile_read": (i32, [vp, vp, vp]),
        "orbx_kernel_name": (C.c_char_p, [i32]),
        "orbx_hamming": (i32, [vp, vp]),
        "orbx_nn_csr": (i32, [vp, vp, i32, vp, i32, vp, vp, i32, vp, vp, vp, vp, vp]),
        "orbx_knn2_allpairs": (i32, [vp, vp, i32, vp, i32, vp, vp]),
        "orbx_nn_csr_device": (i32, [vp, vp, i32, vp, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp]),
        "orbx_knn2_allpairs_device": (i32, [vp, vp, i32, vp, i32, vp, vp, vp]),
        "orbx_features_in_area": (i32, [vp, vp, i32, f32, f32, f32, f32, vp, vp, vp, vp, vp, i32, vp, vp, i32]),
        "orbx_search_for_initialization": (i32, [vp, vp, vp, i32, vp, vp, i32, f32, f32, f32, f32, vp, i32, f32, i32, vp, ip]),
        "orbx_window_search": (i32, [vp, vp, vp, i32, f32, f32, f32, f32, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, i32, vp, vp, vp, vp]),
        "orbx_window_search_grid": (i32, [vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, i32, vp, vp, vp, vp]),
        "orbx_window_nearest": (i32, [vp, vp, vp, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp]),
        "orbx_target_create": (i32, [vp, vp, vp, i32, vp, vp, vp, i32, C.POINTER(C.c_void_p)]),
        "orbx_target_assign": (i32, [vp, vp, vp, vp, i32, vp, vp, vp, i32]),
        "orbx_target_destroy": (None, [vp]),
        "orbx_target_size": (i32, [vp]),
        "orbx_target_search": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, i32, vp, vp, vp, vp]),
        "orbx_target_nearest": (i32, [vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp]),
        "orbx_undistort_keypoints": (i32, [vp, vp, i32, f32, f32, f32, f32, vp, i32, vp]),
        "orbx_undistort_keypoints_device": (i32, [vp, vp, vp, i32, i32, f32, f32, f32, f32, vp, i32, vp, vp]),
        "orbx_search_by_projection": (i32, [vp, vp, vp, vp, vp, i32, f32, f32, f32, f32, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, i32, f32, f32,
                                            vp, ip]),
        "orbx_search_by_projection_last": (i32, [vp, vp, vp, vp, vp, i32, f32, f32, f32, f32, vp, i32, f32, vp, vp, vp, vp, vp, vp, vp, vp, i32,
                                                 f32, i32, i32, vp, ip]),
        "orbx_search_by_bow": (i32, [vp, vp, vp, vp, i32, vp, vp, vp, i32, vp, vp, i32, vp, vp, vp, i32, f32, i32, vp, ip]),
        "orbx_stereo_matches": (i32, [vp, vp, vp, vp, i32, vp, vp, i32, f32, f32, vp, vp, ip]),
        "orbx_voc_load_text": (i32, [vp, C.c_char_p, C.POINTER(vp)]),
        "orbx_voc_create": (i32, [vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, C.POINTER(vp)]),
        "orbx_set_option": (i32, [vp, C.c_char_p, i32]),
        "orbx_get_option": (i32, [vp, C.c_char_p]),
        "orbx_reserve": (i32, [vp, i32, i32, i32]),
        "orbx_voc_save_text": (i32, [vp, C.c_char_p]),
        "orbx_voc_save_binary": (i32, [vp, C.c_char_p]),
        "orbx_voc_load_binary": (i32, [vp, C.c_char_p, C.POINTER(vp)]),
        "orbx_voc_destroy": (None, [vp]),
        "orbx_voc_info": (i32, [vp, ip, ip, ip, ip]),
        "orbx_bow_transform": (i32, [vp, vp, i32, i32, vp, vp, vp]),
        "orbx_bow_transform_published": (i32, [vp, vp, i32, i32, vp, vp, vp]),
        "orbx_nn_groups": (i32, [vp, vp, vp, i32, vp, i32, vp, vp, i32, i32, vp, vp, vp, i32, C.POINTER(C.c_int)]),
        "orbx_bow_transform_device": (i32, [vp, vp, i32, i32, vp, vp, vp, vp]),
        "orbx_bow_finalize": (i32, [vp, vp, vp, i32, vp, vp, ip]),
        "orbx_bow_score_l1": (C.c_double, [vp, vp, i32, vp, vp, i32]),
        "orbx_bow_score_l1_batch": (i32, [vp, vp, vp, i32, vp, vp, vp, i32, vp]),
        "orbx_kfdb_create": (i32, [vp, C.POINTER(vp)]),
        "orbx_kfdb_destroy": (None, [vp]),
        "orbx_kfdb_add": (i32, [vp, C.c_int64, vp, vp, i32]),
        "orbx_kfdb_erase": (i32, [vp, C.c_int64]),
        "orbx_kfdb_clear": (i32, [vp]),
        "orbx_kfdb_size": (i32, [vp]),
        "orbx_kfdb_query": (i32, [vp, vp, vp, i32, vp, i32, i32, vp, vp, vp, i32, ip, ip, ip]),
        "orbx_target_search_view": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp]),
        "orbx_target_search_view_begin": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32]),
        "orbx_target_search_view_end": (i32, [vp, i32, vp, vp]),
        "orbx_target_search_view_cancel": (i32, [vp, i32]),
        "orbx_last_graph_device_us": (C.c_double, [vp]),
        "orbx_last_window_device_us": (C.c_double, [vp]),
        "orbx_publish_descriptors": (i32, [vp, vp, i32]),
        "orbx_kfdb_sharing": (i32, [vp, vp, i32, vp, vp, i32, ip]),
        "orbx_kfdb_score": (i32, [vp, vp, vp, i32, vp, i32, vp]),
        "orbx_cpu_profile_name": (C.c_char_p, [i32]),
        "orbx_cpu_profile_description": (C.c_char_p, [C.c_char_p]),
        "orbx_cpu_profile_values": (i32, [C.c_char_p, i32, vp]),
        "orbx_set_cpu_profile": (i32, [vp, C.c_char_p, i32]),
        "orbx_get_cpu_profile": (i32, [vp, vp, sz, vp]),
        "orbx_replay_unique_id": (i32, [vp]),
        "orbx_replay_rccl_info": (C.c_char_p, []),
        "orbx_replay_create": (i32, [C.POINTER(vp), vp, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp]),
        "orbx_replay_prepare": (i32, [C.POINTER(vp), vp, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp]),
        "orbx_replay_connect": (i32, [vp, vp]),
        "orbx_replay_wait_gathered": (i32, [vp, i32, vp]),
        "orbx_replay_release_gathered": (i32, [vp, i32, vp]),
        "orbx_replay_wait_gathered_host": (i32, [vp, i32, i32]),
        "orbx_replay_failed": (i32, [vp]),
        "orbx_replay_abort": (i32, [vp]),
        "orbx_replay_destroy": (None, [vp]),
        "orbx_replay_last_error": (C.c_char_p, [vp]),
        "orbx_replay_transport": (C.c_char_p, [vp]),
        "orbx_replay_layout": (i32, [vp, ip, ip, C.POINTER(sz), C.POINTER(sz), C.POINTER(sz), C.POINTER(sz), C.POINTER(sz), ip]),
        "orbx_replay_lane_range": (i32, [vp, i32, ip, ip]),
        "orbx_replay_step": (i32, [vp, vp, sz, sz, i32, i32]),
        "orbx_replay_drain": (i32, [vp]),
        "orbx_replay_set_gather": (i32, [vp, i32]),
        "orbx_replay_block": (i32, [vp, i32, C.POINTER(vp)]),
        "orbx_replay_gathered": (i32, [vp, i32, i32, C.POINTER(vp)]),
        "orbx_replay_read": (i32, [vp, i32, i32, vp, sz, sz]),
        "orbx_replay_write_block": (i32, [vp, i32, vp, sz, sz]),
        "orbx_replay_gather_ms": (i32, [vp, C.POINTER(C.c_double), C.POINTER(C.c_longlong), i32]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)  # AttributeError here == header/library mismatch: fail loudly
        fn.restype = res
        fn.argtypes = args
    L._orbx_symbols = tuple(sig)
    # the diagnostic ABI lives in a library of its own (the product has no debug entry point): its functions are bound onto the same object so
    # that the mirrors' debug helpers read `L.orbx_debug_*`; without the library they raise when called
    dsig = {
        "orbx_debug_blur_level": (i32, [vp, i32, i32, vp, sz]),
        "orbx_debug_level_points": (i32, [vp, i32, i32, i32, vp, i32]),
        "orbx_debug_trig": (i32, [vp, vp, vp, i32, i32, vp, vp, vp]),
        "orbx_debug_trig_hash": (i32, [vp, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]),
        "orbx_debug_atan_hash": (i32, [vp, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]),
        "orbx_debug_brief_hash": (i32, [vp, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]),
        "orbx_debug_calib_copy": (i32, [vp, vp, vp, sz, i32, vp]),
        "orbx_debug_gnu_sort": (i32, [vp, vp, i32, i32]),
    }
    L._orbx_debug_symbols = tuple(dsig)
    D = C.CDLL(DEBUG_LIB_PATH) if os.path.exists(DEBUG_LIB_PATH) else None
    for name, (res, args) in dsig.items():
        if D is not None:
            fn = getattr(D, name)
            fn.restype = res
            fn.argtypes = args
        else:
            def fn(*_a, _n=name):
                raise ImportError(f"{_n}: {DEBUG_LIB_PATH} not built (the diagnostic ABI is not part of liborbx.so)")
        setattr(L, name, fn)
    L.HOST_EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t)   # orbx_host_exchange_fn
    _lib = L
    return L


class OrbxTrainParams(C.Structure):
    """orbx_train_params (include/orbx_train.h)."""
    _fields_ = [("k", C.c_int), ("L", C.c_int), ("weighting", C.c_int), ("scoring", C.c_int), ("seed", C.c_uint32),
                ("device_min_node", C.c_int), ("max_iterations", C.c_int)]


class OrbxTrainStats(C.Structure):
    """orbx_train_stats (include/orbx_train.h)."""
    _fields_ = [("device_nodes", C.c_int), ("host_nodes", C.c_int), ("iterations", C.c_int64), ("empty_clusters", C.c_int64),
                ("ms_device", C.c_double), ("ms_host", C.c_double), ("ms_weights", C.c_double), ("ms_create", C.c_double)]

    def as_dict(self) -> dict:
        return {f: getattr(self, f) for f, _ in self._fields_}


ORBX_E_NOCONVERGE = -16
_side = {}


def _load_side(path: str, signatures: dict) -> C.CDLL:
    """A library beside the product, loaded once, with every name of its header bound to its signature (lib() binds exactly include/orbx.h's
    names)."""
    if path in _side:
        return _side[path]
    lib()   # liborbx.so first: the side library resolves its product calls against it
    if not os.path.exists(path):
        raise ImportError(f"{path} not built — run `python -m orb_slam3_modified_amd.build`")
    S = C.CDLL(path)
    for name, (res, args) in signatures.items():
        fn = getattr(S, name)   # AttributeError here == header/library mismatch: fail loudly
        fn.restype = res
        fn.argtypes = args
    _side[path] = S
    return S


def train_lib() -> C.CDLL:
    """liborbx_train.so (include/orbx_train.h)."""
    vp = C.c_void_p
    return _load_side(TRAIN_LIB_PATH, {
        "orbx_train_vocabulary": (C.c_int, [vp, vp, vp, C.c_int, C.POINTER(OrbxTrainParams), C.POINTER(vp), C.POINTER(OrbxTrainStats)]),
        "orbx_train_last_error": (C.c_char_p, []),
        "orbx_train_glibc_rand": (C.c_int, [C.c_uint32, C.c_int, vp]),
    })


def stereo_lib() -> C.CDLL:
    """liborbx_stereo.so.  `_orbx_stereo_symbols`: every name of include/orbx_stereo.h, bound here with its signature."""
    vp, i32, sz, f32 = C.c_void_p, C.c_int, C.c_size_t, C.c_float
    sig = {
        "orbx_stereo_create": (i32, [C.POINTER(vp), vp, vp, f32, f32]),
        "orbx_stereo_destroy": (None, [vp]),
        "orbx_stereo_last_error": (C.c_char_p, [vp]),
        "orbx_stereo_match_batch_device": (i32, [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "orbx_stereo_extract_batch_device": (i32, [vp, vp, vp, i32, i32, i32, sz, sz, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "orbx_stereo_extract_batch": (i32, [vp, vp, vp, i32, i32, i32, sz, sz, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    }
    S = _load_side(STEREO_LIB_PATH, sig)
    S._orbx_stereo_symbols = tuple(sig)
    return S


def bow_lib() -> C.CDLL:
    """liborbx_bow.so.  `_orbx_bow_symbols`: every name of include/orbx_bow.h, bound here with its signature."""
    vp, i32 = C.c_void_p, C.c_int
    sig = {
        "orbx_bow_create": (i32, [C.POINTER(vp), vp, i32]),
        "orbx_bow_destroy": (None, [vp]),
        "orbx_bow_last_error": (C.c_char_p, [vp]),
        "orbx_bow_transform_batch_device": (i32, [vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp]),
        "orbx_bow_transform_batch": (i32, [vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp]),
        "orbx_bow_score_matrix_device": (i32, [vp, vp, vp, vp, i32, i32, vp, vp, vp, i32, i32, vp, vp]),
        "orbx_bow_score_matrix": (i32, [vp, vp, vp, vp, i32, vp, vp, vp, i32, vp]),
    }
    B = _load_side(BOW_LIB_PATH, sig)
    B._orbx_bow_symbols = tuple(sig)
    return B


class OrbxMatchSide(C.Structure):
    """orbx_match_side (include/orbx_match.h)."""
    _fields_ = [("d_kps", C.c_void_p), ("d_desc", C.c_void_p), ("d_counts", C.c_void_p), ("d_fv_node", C.c_void_p), ("d_fv_ptr", C.c_void_p),
                ("d_fv_feat", C.c_void_p), ("d_fv_n", C.c_void_p), ("d_valid", C.c_void_p), ("nframes", C.c_int), ("capacity", C.c_int)]


def match_lib() -> C.CDLL:
    """liborbx_match.so.  `_orbx_match_symbols`: every name of include/orbx_match.h, bound here with its signature."""
    vp, i32, f32, sp = C.c_void_p, C.c_int, C.c_float, C.POINTER(OrbxMatchSide)
    sig = {
        "orbx_match_create": (i32, [C.POINTER(vp), i32]),
        "orbx_match_destroy": (None, [vp]),
        "orbx_match_last_error": (C.c_char_p, [vp]),
        "orbx_match_bow_pairs_device": (i32, [vp, sp, sp, vp, i32, i32, f32, i32, vp, vp, vp, vp]),
        "orbx_match_bow_pairs": (i32, [vp, sp, sp, vp, i32, i32, f32, i32, vp, vp, vp]),
    }
    M = _load_side(MATCH_LIB_PATH, sig)
    M._orbx_match_symbols = tuple(sig)
    return M


class OrbxInitMatchSide(C.Structure):
    """orbx_initmatch_side (include/orbx_initmatch.h)."""
    _fields_ = [("d_kps", C.c_void_p), ("d_desc", C.c_void_p), ("d_counts", C.c_void_p), ("nframes", C.c_int), ("capacity", C.c_int)]


def initmatch_lib(path: str = INITMATCH_LIB_PATH) -> C.CDLL:
    """liborbx_initmatch.so.  `_orbx_initmatch_symbols`: every name of include/orbx_initmatch.h, bound here with its signature.  `path`: a
    timing build of the same source (tools/initmatch_times.py)."""
    vp, i32, f32, sp, fp = C.c_void_p, C.c_int, C.c_float, C.POINTER(OrbxInitMatchSide), C.POINTER(C.c_float)
    sig = {
        "orbx_initmatch_create": (i32, [C.POINTER(vp), i32]),
        "orbx_initmatch_destroy": (None, [vp]),
        "orbx_initmatch_last_error": (C.c_char_p, [vp]),
        "orbx_initmatch_pairs_device": (i32, [vp, sp, sp, vp, i32, fp, i32, f32, i32, vp, vp, vp, vp, vp]),
        "orbx_initmatch_pairs": (i32, [vp, sp, sp, vp, i32, fp, i32, f32, i32, vp, vp, vp, vp]),
    }
    M = _load_side(path, sig)
    M._orbx_initmatch_symbols = tuple(sig)
    return M


class OrbxTriMatchSide(C.Structure):
    """orbx_trimatch_side (include/orbx_trimatch.h)."""
    _fields_ = [("d_kps", C.c_void_p), ("d_desc", C.c_void_p), ("d_counts", C.c_void_p), ("d_fv_node", C.c_void_p), ("d_fv_ptr", C.c_void_p),
                ("d_fv_feat", C.c_void_p), ("d_fv_n", C.c_void_p), ("d_has_point", C.c_void_p), ("d_uright", C.c_void_p), ("nframes", C.c_int),
                ("capacity", C.c_int)]


def trimatch_lib() -> C.CDLL:
    """liborbx_trimatch.so.  `_orbx_trimatch_symbols`: every name of include/orbx_trimatch.h, bound here with its signature."""
    vp, i32, sp, fp = C.c_void_p, C.c_int, C.POINTER(OrbxTriMatchSide), C.POINTER(C.c_float)
    sig = {
        "orbx_trimatch_create": (i32, [C.POINTER(vp), i32]),
        "orbx_trimatch_destroy": (None, [vp]),
        "orbx_trimatch_last_error": (C.c_char_p, [vp]),
        "orbx_trimatch_pairs_device": (i32, [vp, sp, sp, vp, i32, vp, fp, fp, i32, i32, i32, i32, vp, vp, vp]),
        "orbx_trimatch_pairs": (i32, [vp, sp, sp, vp, i32, vp, fp, fp, i32, i32, i32, i32, vp, vp]),
    }
    M = _load_side(TRIMATCH_LIB_PATH, sig)
    M._orbx_trimatch_symbols = tuple(sig)
    return M


class OrbxFuseSide(C.Structure):
    """orbx_fuse_side (include/orbx_fuse.h)."""
    _fields_ = [("d_kps", C.c_void_p), ("d_desc", C.c_void_p), ("d_counts", C.c_void_p), ("d_uright", C.c_void_p), ("d_gridparm", C.c_void_p),
                ("nframes", C.c_int), ("capacity", C.c_int)]


def fuse_lib() -> C.CDLL:
    """liborbx_fuse.so.  `_orbx_fuse_symbols`: every name of include/orbx_fuse.h, bound here with its signature."""
    vp, i32, sp, fp = C.c_void_p, C.c_int, C.POINTER(OrbxFuseSide), C.POINTER(C.c_float)
    sig = {
        "orbx_fuse_create": (i32, [C.POINTER(vp), i32]),
        "orbx_fuse_destroy": (None, [vp]),
        "orbx_fuse_last_error": (C.c_char_p, [vp]),
        "orbx_fuse_grids_device": (i32, [vp, sp, vp]),
        "orbx_fuse_search_device": (i32, [vp, sp, vp, vp, i32, vp, i32, vp, i32, fp, i32, i32, i32, vp, vp, vp, vp]),
        "orbx_fuse_search": (i32, [vp, sp, vp, vp, i32, vp, i32, vp, i32, fp, i32, i32, i32, vp, vp, vp]),
    }
    M = _load_side(FUSE_LIB_PATH, sig)
    M._orbx_fuse_symbols = tuple(sig)
    return M


class OrbxMpdescSide(C.Structure):
    """orbx_mpdesc_side (include/orbx_mpdesc.h)."""
    _fields_ = [("d_desc", C.c_void_p), ("d_counts", C.c_void_p), ("nframes", C.c_int), ("capacity", C.c_int)]


def mpdesc_lib() -> C.CDLL:
    """liborbx_mpdesc.so.  `_orbx_mpdesc_symbols`: every name of include/orbx_mpdesc.h, bound here with its signature."""
    vp, i32, sp = C.c_void_p, C.c_int, C.POINTER(OrbxMpdescSide)
    sig = {
        "orbx_mpdesc_create": (i32, [C.POINTER(vp), i32]),
        "orbx_mpdesc_destroy": (None, [vp]),
        "orbx_mpdesc_last_error": (C.c_char_p, [vp]),
        "orbx_mpdesc_select_device": (i32, [vp, sp, vp, i32, vp, i32, vp, vp, i32, vp, vp, vp]),
        "orbx_mpdesc_select": (i32, [vp, sp, vp, i32, vp, i32, vp, vp, i32, vp, vp]),
    }
    M = _load_side(MPDESC_LIB_PATH, sig)
    M._orbx_mpdesc_symbols = tuple(sig)
    return M


def score_lib() -> C.CDLL:
    """liborbx_score.so.  `_orbx_score_symbols`: every name of include/orbx_score.h, bound here with its signature."""
    vp, i32 = C.c_void_p, C.c_int
    sig = {
        "orbx_score_create": (i32, [C.POINTER(vp), i32]),
        "orbx_score_destroy": (None, [vp]),
        "orbx_score_last_error": (C.c_char_p, [vp]),
        "orbx_score_pair": (C.c_double, [i32, vp, vp, i32, vp, vp, i32]),
        "orbx_score_matrix_device": (i32, [vp, i32, vp, vp, vp, i32, i32, vp, vp, vp, i32, i32, vp, vp]),
        "orbx_score_matrix": (i32, [vp, i32, vp, vp, vp, i32, vp, vp, vp, i32, vp]),
    }
    M = _load_side(SCORE_LIB_PATH, sig)
    M._orbx_score_symbols = tuple(sig)
    return M


def fisheye_lib() -> C.CDLL:
    """liborbx_fisheye.so.  `_orbx_fisheye_symbols`: every name of include/orbx_fisheye.h, bound here with its signature."""
    vp, i32, sz = C.c_void_p, C.c_int, C.c_size_t
    sig = {
        "orbx_fisheye_create": (i32, [C.POINTER(vp), vp, vp]),
        "orbx_fisheye_destroy": (None, [vp]),
        "orbx_fisheye_last_error": (C.c_char_p, [vp]),
        "orbx_fisheye_match_batch_device": (i32, [vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "orbx_fisheye_finish_batch_device": (i32, [vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "orbx_fisheye_extract_batch_device": (i32, [vp, vp, vp, i32, i32, i32, sz, sz, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                                    vp]),
        "orbx_fisheye_match_batch": (i32, [vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp]),
        "orbx_fisheye_finish_batch": (i32, [vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    }
    M = _load_side(FISHEYE_LIB_PATH, sig)
    M._orbx_fisheye_symbols = tuple(sig)
    return M


class OrbxLocalMatchSide(C.Structure):
    """orbx_localmatch_side (include/orbx_localmatch.h)."""
    _fields_ = [("d_kps", C.c_void_p), ("d_desc", C.c_void_p), ("d_counts", C.c_void_p), ("d_uright", C.c_void_p), ("d_bounds", C.c_void_p),
                ("nframes", C.c_int), ("capacity", C.c_int)]


def localmatch_lib(path: str = LOCALMATCH_LIB_PATH) -> C.CDLL:
    """liborbx_localmatch.so.  `_orbx_localmatch_symbols`: every name of include/orbx_localmatch.h, bound here with its signature.  `path`: a
    timing build of the same source (tools/localmatch_times.py)."""
    vp, i32, f32, sp, fp = C.c_void_p, C.c_int, C.c_float, C.POINTER(OrbxLocalMatchSide), C.POINTER(C.c_float)
    sig = {
        "orbx_localmatch_create": (i32, [C.POINTER(vp), i32]),
        "orbx_localmatch_destroy": (None, [vp]),
        "orbx_localmatch_last_error": (C.c_char_p, [vp]),
        "orbx_localmatch_search_device": (i32, [vp, sp, vp, i32, vp, vp, i32, vp, i32, fp, i32, f32, f32, vp, vp, vp, vp]),
        "orbx_localmatch_search": (i32, [vp, sp, vp, i32, vp, vp, i32, vp, i32, fp, i32, f32, f32, vp, vp, vp]),
    }
    M = _load_side(path, sig)
    M._orbx_localmatch_symbols = tuple(sig)
    return M


class OrbxLastMatchSide(C.Structure):
    """orbx_lastmatch_side (include/orbx_lastmatch.h)."""
    _fields_ = [("d_kps", C.c_void_p), ("d_desc", C.c_void_p), ("d_counts", C.c_void_p), ("d_uright", C.c_void_p), ("d_bounds", C.c_void_p),
                ("nframes", C.c_int), ("capacity", C.c_int)]


def lastmatch_lib(path: str = LASTMATCH_LIB_PATH) -> C.CDLL:
    """liborbx_lastmatch.so.  `_orbx_lastmatch_symbols`: every name of include/orbx_lastmatch.h, bound here with its signature.  `path`: a
    timing build of the same source (tools/lastmatch_times.py)."""
    vp, i32, sp, fp = C.c_void_p, C.c_int, C.POINTER(OrbxLastMatchSide), C.POINTER(C.c_float)
    sig = {
        "orbx_lastmatch_create": (i32, [C.POINTER(vp), i32]),
        "orbx_lastmatch_destroy": (None, [vp]),
        "orbx_lastmatch_last_error": (C.c_char_p, [vp]),
        "orbx_lastmatch_search_device": (i32, [vp, sp, vp, i32, vp, vp, i32, vp, i32, fp, i32, i32, vp, vp, vp, vp]),
        "orbx_lastmatch_search": (i32, [vp, sp, vp, i32, vp, vp, i32, vp, i32, fp, i32, i32, vp, vp, vp]),
    }
    M = _load_side(path, sig)
    M._orbx_lastmatch_symbols = tuple(sig)
    return M


class OrbxProjMatchSide(C.Structure):
    """orbx_projmatch_side (include/orbx_projmatch.h)."""
    _fields_ = [("d_kps", C.c_void_p), ("d_desc", C.c_void_p), ("d_counts", C.c_void_p), ("d_bounds", C.c_void_p), ("nframes", C.c_int),
                ("capacity", C.c_int)]


def projmatch_lib(path: str = PROJMATCH_LIB_PATH) -> C.CDLL:
    """liborbx_projmatch.so.  `_orbx_projmatch_symbols`: every name of include/orbx_projmatch.h, bound here with its signature.  `path`: a
    timing build of the same source (tools/projmatch_times.py)."""
    vp, i32, sp, fp = C.c_void_p, C.c_int, C.POINTER(OrbxProjMatchSide), C.POINTER(C.c_float)
    sig = {
        "orbx_projmatch_create": (i32, [C.POINTER(vp), i32]),
        "orbx_projmatch_destroy": (None, [vp]),
        "orbx_projmatch_last_error": (C.c_char_p, [vp]),
        "orbx_projmatch_search_device": (i32, [vp, sp, vp, i32, vp, vp, i32, vp, i32, fp, i32, i32, vp, vp, vp, vp]),
        "orbx_projmatch_search": (i32, [vp, sp, vp, i32, vp, vp, i32, vp, i32, fp, i32, i32, vp, vp, vp]),
    }
    M = _load_side(path, sig)
    M._orbx_projmatch_symbols = tuple(sig)
    return M


class OrbxPlaceDb(C.Structure):
    """orbx_place_db (include/orbx_place.h)."""
    _fields_ = [("d_ids", C.c_void_p), ("d_vals", C.c_void_p), ("d_n", C.c_void_p), ("d_kf_map", C.c_void_p), ("d_kf_cov", C.c_void_p),
                ("d_kf_score", C.c_void_p), ("count", C.c_int), ("stride", C.c_int)]


class OrbxPlaceQueries(C.Structure):
    """orbx_place_queries (include/orbx_place.h)."""
    _fields_ = [("d_ids", C.c_void_p), ("d_vals", C.c_void_p), ("d_n", C.c_void_p), ("d_q_map", C.c_void_p), ("d_excl_ptr", C.c_void_p),
                ("d_excl_idx", C.c_void_p), ("count", C.c_int), ("stride", C.c_int), ("n_excl", C.c_int)]


def place_lib(path: str = PLACE_LIB_PATH) -> C.CDLL:
    """liborbx_place.so.  `_orbx_place_symbols`: every name of include/orbx_place.h, bound here with its signature.  `path`: a timing build
    of the same source (tools/place_times.py)."""
    vp, i32, dp, qp = C.c_void_p, C.c_int, C.POINTER(OrbxPlaceDb), C.POINTER(OrbxPlaceQueries)
    sig = {
        "orbx_place_create": (i32, [C.POINTER(vp), i32]),
        "orbx_place_destroy": (None, [vp]),
        "orbx_place_last_error": (C.c_char_p, [vp]),
        "orbx_place_query_device": (i32, [vp, i32, i32, dp, qp, i32, vp, vp, vp, vp, vp, vp]),
        "orbx_place_query": (i32, [vp, i32, i32, dp, qp, i32, vp, vp, vp, vp, vp]),
    }
    M = _load_side(path, sig)
    M._orbx_place_symbols = tuple(sig)
    return M


def placeindex_lib(path: str = PLACEINDEX_LIB_PATH) -> C.CDLL:
    """liborbx_placeindex.so.  `_orbx_placeindex_symbols`: every name of include/orbx_placeindex.h, bound here with its signature.  `path`: a
    timing build of the same source (tools/placeindex_times.py)."""
    vp, i32, dp, qp = C.c_void_p, C.c_int, C.POINTER(OrbxPlaceDb), C.POINTER(OrbxPlaceQueries)
    sig = {
        "orbx_placeindex_create": (i32, [C.POINTER(vp), i32, i32]),
        "orbx_placeindex_destroy": (None, [vp]),
        "orbx_placeindex_last_error": (C.c_char_p, [vp]),
        "orbx_placeindex_sync_device": (i32, [vp, dp, vp]),
        "orbx_placeindex_query_device": (i32, [vp, i32, i32, dp, qp, i32, vp, vp, vp, vp, vp, vp]),
        "orbx_placeindex_query": (i32, [vp, i32, i32, dp, qp, i32, vp, vp, vp, vp, vp]),
    }
    M = _load_side(path, sig)
    M._orbx_placeindex_symbols = tuple(sig)
    return M


def frustum_lib(path: str = FRUSTUM_LIB_PATH) -> C.CDLL:
    """liborbx_frustum.so.  `_orbx_frustum_symbols`: every name of include/orbx_frustum.h, bound here with its signature.  `path`: a timing
    build of the same source."""
    vp, i32, f32 = C.c_void_p, C.c_int, C.c_float
    call = [vp, vp, i32, vp, i32, vp, vp, i32, f32, i32, f32, i32, i32, vp, vp, vp]   # points .. ntomatch
    sig = {
        "orbx_frustum_create": (i32, [C.POINTER(vp), i32]),
        "orbx_frustum_destroy": (None, [vp]),
        "orbx_frustum_last_error": (C.c_char_p, [vp]),
        "orbx_frustum_level_thresholds": (i32, [f32, i32, i32, vp]),
        "orbx_frustum_project_device": (i32, [vp] + call + [vp]),
        "orbx_frustum_project": (i32, [vp] + call),
        "orbx_frustum_project_reference": (i32, call),
    }
    M = _load_side(path, sig)
    M._orbx_frustum_symbols = tuple(sig)
    return M


def project_lib(path: str = PROJECT_LIB_PATH) -> C.CDLL:
    """liborbx_project.so.  `_orbx_project_symbols`: every name of include/orbx_project.h, bound here with its signature.  `path`: a timing
    build of the same source."""
    vp, i32, f32 = C.c_void_p, C.c_int, C.c_float
    head, tail = [vp, i32, vp, i32, vp, vp, i32], [i32, i32, vp, vp]   # points, npoints .. mcap; rot_kind .. nvalid
    last = [vp, vp, i32, vp, i32, vp, vp, i32] + tail                  # with obs
    sig = {
        "orbx_project_create": (i32, [C.POINTER(vp), i32]),
        "orbx_project_destroy": (None, [vp]),
        "orbx_project_last_error": (C.c_char_p, [vp]),
        "orbx_project_last_device": (i32, [vp] + last + [vp]),
        "orbx_project_last": (i32, [vp] + last),
        "orbx_project_last_reference": (i32, last),
        "orbx_project_reloc_device": (i32, [vp] + head + [vp, i32] + tail + [vp]),
        "orbx_project_reloc": (i32, [vp] + head + [vp, i32] + tail),
        "orbx_project_reloc_reference": (i32, head + [f32, i32, i32] + tail),
        "orbx_project_fuse_device": (i32, [vp] + head + [vp, vp, i32] + tail + [vp]),
        "orbx_project_fuse": (i32, [vp] + head + [vp, vp, i32] + tail),
        "orbx_project_fuse_reference": (i32, head + [f32, vp, i32, i32] + tail),
    }
    M = _load_side(path, sig)
    M._orbx_project_symbols = tuple(sig)
    return M


def sim3_lib(path: str = SIM3_LIB_PATH) -> C.CDLL:
    """liborbx_sim3.so.  `_orbx_sim3_symbols`: every name of include/orbx_sim3.h, bound here with its signature.  `path`: a timing build of
    the same source."""
    vp, i32, f32 = C.c_void_p, C.c_int, C.c_float
    head, tail = [vp, i32, vp, i32, vp, vp, i32], [i32, i32, vp, vp]   # points, npoints .. mcap; rot_kind, sum_order, out, nvalid
    stail = [i32, i32, i32, vp, vp]                                    # search: with sim_kind
    agree = [vp] * 8 + [i32, i32, i32, vp, vp]
    sig = {
        "orbx_sim3_create": (i32, [C.POINTER(vp), i32]),
        "orbx_sim3_destroy": (None, [vp]),
        "orbx_sim3_last_error": (C.c_char_p, [vp]),
        "orbx_sim3_proj_device": (i32, [vp] + head + [vp, i32, i32] + tail + [vp]),   # thresholds, nlevels, proj_kind
        "orbx_sim3_proj": (i32, [vp] + head + [vp, i32, i32] + tail),
        "orbx_sim3_proj_reference": (i32, head + [f32, i32, i32, i32] + tail),
        "orbx_sim3_fuse_device": (i32, [vp] + head + [vp, vp, i32] + tail + [vp]),
        "orbx_sim3_fuse": (i32, [vp] + head + [vp, vp, i32] + tail),
        "orbx_sim3_fuse_reference": (i32, head + [f32, vp, i32, i32] + tail),
        "orbx_sim3_search_device": (i32, [vp] + head + [vp, vp, i32] + stail + [vp]),
        "orbx_sim3_search": (i32, [vp] + head + [vp, vp, i32] + stail),
        "orbx_sim3_search_reference": (i32, head + [f32, vp, i32, i32] + stail),
        "orbx_sim3_agree_device": (i32, [vp] + agree + [vp]),
        "orbx_sim3_agree": (i32, [vp] + agree),
        "orbx_sim3_agree_reference": (i32, agree),
    }
    M = _load_side(path, sig)
    M._orbx_sim3_symbols = tuple(sig)
    return M


class OrbxRigMatchSide(C.Structure):
    """orbx_rigmatch_side (include/orbx_rigmatch.h)."""
    _fields_ = [("d_kps_l", C.c_void_p), ("d_desc_l", C.c_void_p), ("d_counts_l", C.c_void_p), ("d_kps_r", C.c_void_p), ("d_desc_r", C.c_void_p),
                ("d_counts_r", C.c_void_p), ("d_l2r", C.c_void_p), ("d_r2l", C.c_void_p), ("d_bounds", C.c_void_p), ("nframes", C.c_int),
                ("cap_l", C.c_int), ("cap_r", C.c_int)]


def rigmatch_lib(path: str = RIGMATCH_LIB_PATH) -> C.CDLL:
    """liborbx_rigmatch.so.  `_orbx_rigmatch_symbols`: every name of include/orbx_rigmatch.h, bound here with its signature.  `path`: a
    timing build of the same source."""
    vp, i32, f32, sp, fp = C.c_void_p, C.c_int, C.c_float, C.POINTER(OrbxRigMatchSide), C.POINTER(C.c_float)
    sig = {
        "orbx_rigmatch_create": (i32, [C.POINTER(vp), i32]),
        "orbx_rigmatch_destroy": (None, [vp]),
        "orbx_rigmatch_last_error": (C.c_char_p, [vp]),
        "orbx_rigmatch_local_device": (i32, [vp, sp, vp, i32, vp, vp, i32, vp, i32, fp, i32, f32, f32, vp, vp, vp, vp]),
        "orbx_rigmatch_local": (i32, [vp, sp, vp, i32, vp, vp, i32, vp, i32, fp, i32, f32, f32, vp, vp, vp]),
        "orbx_rigmatch_last_device": (i32, [vp, sp, vp, i32, vp, vp, i32, vp, i32, fp, i32, i32, vp, vp, vp, vp]),
        "orbx_rigmatch_last": (i32, [vp, sp, vp, i32, vp, vp, i32, vp, i32, fp, i32, i32, vp, vp, vp]),
    }
    M = _load_side(path, sig)
    M._orbx_rigmatch_symbols = tuple(sig)
    return M


class OrbxRigBowRig(C.Structure):
    """orbx_rigbow_rig (include/orbx_rigbow.h)."""
    _fields_ = [("d_kps_l", C.c_void_p), ("d_desc_l", C.c_void_p), ("d_counts_l", C.c_void_p), ("d_kps_r", C.c_void_p), ("d_desc_r", C.c_void_p),
                ("d_counts_r", C.c_void_p), ("nframes", C.c_int), ("cap_l", C.c_int), ("cap_r", C.c_int)]


class OrbxRigBowSide(C.Structure):
    """orbx_rigbow_side (include/orbx_rigbow.h)."""
    _fields_ = [("d_kps", C.c_void_p), ("d_desc", C.c_void_p), ("d_counts", C.c_void_p), ("d_fv_node", C.c_void_p), ("d_fv_ptr", C.c_void_p),
                ("d_fv_feat", C.c_void_p), ("d_fv_n", C.c_void_p), ("d_valid", C.c_void_p), ("d_nleft", C.c_void_p), ("nframes", C.c_int),
                ("capacity", C.c_int)]


def rigbow_lib(path: str = RIGBOW_LIB_PATH) -> C.CDLL:
    """liborbx_rigbow.so.  `_orbx_rigbow_symbols`: every name of include/orbx_rigbow.h, bound here with its signature.  `path`: a timing
    build of the same source."""
    vp, i32, f32, sp, rp = C.c_void_p, C.c_int, C.c_float, C.POINTER(OrbxRigBowSide), C.POINTER(OrbxRigBowRig)
    sig = {
        "orbx_rigbow_create": (i32, [C.POINTER(vp), i32]),
        "orbx_rigbow_destroy": (None, [vp]),
        "orbx_rigbow_last_error": (C.c_char_p, [vp]),
        "orbx_rigbow_stack_device": (i32, [vp, rp, i32, vp, vp, vp, vp, vp]),
        "orbx_rigbow_pairs_device": (i32, [vp, sp, sp, vp, i32, i32, f32, i32, vp, vp, vp, vp]),
        "orbx_rigbow_pairs": (i32, [vp, sp, sp, vp, i32, i32, f32, i32, vp, vp, vp]),
    }
    M = _load_side(path, sig)
    M._orbx_rigbow_symbols = tuple(sig)
    return M


class OrbxMpgeomSide(C.Structure):
    """orbx_mpgeom_side (include/orbx_mpgeom.h)."""
    _fields_ = [("d_kps", C.c_void_p), ("d_counts", C.c_void_p), ("d_nleft", C.c_void_p), ("d_centres", C.c_void_p), ("nframes", C.c_int),
                ("capacity", C.c_int)]


def mpgeom_lib(path: str = MPGEOM_LIB_PATH) -> C.CDLL:
    """liborbx_mpgeom.so.  `_orbx_mpgeom_symbols`: every name of include/orbx_mpgeom.h, bound here with its signature.  `path`: a timing
    build of the same source."""
    vp, i32, sp = C.c_void_p, C.c_int, C.POINTER(OrbxMpgeomSide)
    call = [sp, vp, i32, vp, i32, vp, vp, vp, i32, vp, i32, i32, i32, vp, vp]   # side .. min_dist
    sig = {
        "orbx_mpgeom_create": (i32, [C.POINTER(vp), i32]),
        "orbx_mpgeom_destroy": (None, [vp]),
        "orbx_mpgeom_last_error": (C.c_char_p, [vp]),
        "orbx_mpgeom_update_device": (i32, [vp] + call + [vp]),
        "orbx_mpgeom_update": (i32, [vp] + call),
        "orbx_mpgeom_update_reference": (i32, call),
    }
    M = _load_side(path, sig)
    M._orbx_mpgeom_symbols = tuple(sig)
    return M


class SideHandle:
    """A handle of a side library whose entry points are <prefix>_create / _destroy / _last_error (StereoBatch, BowBatch, MatchBatch,
    InitMatchBatch, TriMatchBatch, FuseBatch, DistinctBatch, ScoreBatch, FisheyeBatch, LocalMatchBatch, LastMatchBatch, ProjMatchBatch,
    PlaceBatch, PlaceIndex, FrustumBatch, ProjectBatch, Sim3Batch, RigMatchBatch, RigBowBatch, NormalDepthBatch)."""

    def __init__(self, library: C.CDLL, prefix: str, *create_args):
        self._L, self._prefix, self._h = library, prefix, C.c_void_p(0)
        rc = self._fn("create")(C.byref(self._h), *create_args)
        if rc != 0:
            raise OrbxError(rc, self._last_error(None))

    def _fn(self, name: str):
        return getattr(self._L, f"{self._prefix}_{name}")

    def _last_error(self, handle) -> str:
        m = self._fn("last_error")(handle)
        return m.decode() if m else ""

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._fn("destroy")(self._h)
            self._h = C.c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int) -> int:
        if rc < 0:
            raise OrbxError(rc, self._last_error(self._h))
        return rc


class OrbxGrid(C.Structure):
    """orbx_grid (include/orbx.h): a Frame's / KeyFrame's feature grid as the caller holds it."""
    _fields_ = [("min_x", C.c_float), ("min_y", C.c_float), ("inv_w", C.c_float), ("inv_h", C.c_float),
                ("cell_start", C.c_void_p), ("cell_idx", C.c_void_p)]


def ptr(a) -> C.c_void_p:
    """void* of a numpy array, an int address, or None."""
    if a is None:
        return C.c_void_p(0)
    if isinstance(a, np.ndarray):
        return a.ctypes.data_as(C.c_void_p)
    return C.c_void_p(int(a))


def addr(t) -> int:
    """An address: a torch tensor's data_ptr(), a numpy array's buffer, an int, or None (0)."""
    if t is None:
        return 0
    if isinstance(t, np.ndarray):
        return int(t.ctypes.data)
    return int(t.data_ptr()) if hasattr(t, "data_ptr") else int(t)


def host_array(x, dtype, *shape) -> np.ndarray:
    """A contiguous numpy array of the ABI's element type and shape."""
    return np.ascontiguousarray(x, dtype).reshape(shape)


def host_view(t):
    """A result (or a row of one) on the host: a numpy array as it is, a torch tensor copied, None as None."""
    return None if t is None else (t if isinstance(t, np.ndarray) else t.cpu().numpy())


def check(rc: int, ctx=None) -> int:
    if rc < 0:
        msg = ""
        if ctx:
            m = lib().orbx_last_error(ctx)
            msg = m.decode() if m else ""
        raise OrbxError(rc, msg)
    return rc
