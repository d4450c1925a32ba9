"""ctypes loader of libzkmi355x.so -- the HIP product library (include/zkmi355x.h).

There is no CPU fallback: if the shared object is missing, or no MI355X is visible when a
compute entry point is called, the error is raised to the caller.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# ZK_LIBZKMI355X_PATH: load another build of the SAME library (the host-only sanitizer build of `make asan-host`, tests/test_sanitizers.py).
# Not a fallback: a missing file or a missing entry point still fails loudly.
LIB_PATH = os.environ.get("ZK_LIBZKMI355X_PATH") or os.path.join(_HERE, "libzkmi355x.so")

# every symbol include/zkmi355x.h declares (checked by tests/test_abi.py without a GPU)
EXPORTS = [
    "zk_strerror", "zk_last_error", "zk_device_count", "zk_init", "zk_shutdown", "zk_set_devices", "zk_set_device_list", "zk_get_device_list", "zk_set_option",
    "zk_fr_ntt", "zk_fr_poly_mul", "zk_fr_spmv", "zk_fr_lagrange_at", "zk_msm_g1", "zk_msm_g2",
    "zk_bases_upload", "zk_bases_info", "zk_bases_free", "zk_msm_resident", "zk_msm_resident_many", "zk_g1_of_fr", "zk_g2_of_fr",
    "zk_g1_powers", "zk_g2_powers", "zk_g1_compress", "zk_g2_compress", "zk_g1_decompress", "zk_g2_decompress", "zk_g1_decompress_batch", "zk_g2_decompress_batch",
    "zk_groth16_pk_upload", "zk_groth16_pk_upload_lagrange", "zk_groth16_pk_derive_lagrange", "zk_groth16_lagrange_pool_sizes", "zk_groth16_pk_derive_lagrange_sets", "zk_groth16_pk_install_lagrange", "zk_groth16_pk_shard", "zk_groth16_shard_range", "zk_groth16_pool_points", "zk_groth16_pk_free", "zk_groth16_prove", "zk_groth16_reserve_slots", "zk_groth16_prove_async", "zk_groth16_prove_wait", "zk_groth16_set_witness", "zk_groth16_qap_eval",
    "zk_groth16_pk_upload_sharded", "zk_groth16_prove_partial", "zk_groth16_prove_partial_async", "zk_groth16_prove_partial_wait", "zk_groth16_combine", "zk_groth16_prove_partial_wait_device", "zk_groth16_combine_device",
    "zk_groth16_pool_layout", "zk_groth16_scalars_async", "zk_groth16_scalars_wait", "zk_groth16_msm_partial_async",
    "zk_device_malloc", "zk_device_free", "zk_device_memcpy",
    "zk_pinocchio_pk_upload", "zk_pinocchio_pk_derive_lagrange", "zk_pinocchio_pool_points", "zk_pinocchio_pk_free", "zk_pinocchio_prove",
    "zk_pinocchio_reserve_slots", "zk_pinocchio_set_witness", "zk_pinocchio_prove_async", "zk_pinocchio_prove_wait",
    "zk_groth16_keygen", "zk_pinocchio_keygen", "zk_pinocchio_pk_upload_lagrange",
    "zk_pairing_product", "zk_pairing_check", "zk_groth16_verify", "zk_pinocchio_verify",
    "zk_pairing_product_many", "zk_groth16_verify_many", "zk_pinocchio_verify_many",
    "zk_groth16_vk_upload", "zk_pinocchio_vk_upload", "zk_vk_info", "zk_vk_free", "zk_groth16_verify_resident", "zk_pinocchio_verify_resident",
    "zk_groth16_verify_folded", "zk_pinocchio_verify_folded",
    "zk_groth16_verify_resident_compressed", "zk_pinocchio_verify_resident_compressed", "zk_groth16_verify_folded_compressed", "zk_pinocchio_verify_folded_compressed",
    "zk_profile_enable", "zk_profile_reset", "zk_profile_get", "zk_profile_names", "zk_profile_counter", "zk_sync",
    "zk_bench_field_mul", "zk_selftest_fp", "zk_selftest_fp_paired", "zk_selftest_fp2_lanewise", "zk_selftest_sqrt", "zk_selftest_fp12", "zk_selftest_subgroup", "zk_selftest_groth16_fold", "zk_selftest_pinocchio_fold", "zk_selftest_group", "zk_selftest_point_decompress",
    "zk_selftest_fr", "zk_selftest_fr29", "zk_selftest_fp29",
    "zk_groth16_pk_upload_compressed", "zk_pinocchio_pk_upload_compressed", "zk_bases_upload_compressed", "zk_groth16_pool_points_compressed", "zk_pinocchio_pool_points_compressed",
    "zk_groth16_prove_many_compressed", "zk_pinocchio_prove_many_compressed", "zk_selftest_proof_wire",
    "zk_groth16_key_check", "zk_groth16_key_check_lagrange",
    "zk_groth16_pk_contribute", "zk_selftest_g1_scale",
    "zk_groth16_srs_sizes", "zk_groth16_pk_specialize", "zk_selftest_g1_colsum",
    "zk_groth16_srs_check", "zk_groth16_srs_contribute",
]


class ZkError(RuntimeError):
    def __init__(self, code, detail):
        self.code = code
        super().__init__("libzkmi355x error %d: %s" % (code, detail))


class CSR(C.Structure):
    _fields_ = [("row_ptr", C.POINTER(C.c_uint32)), ("col", C.POINTER(C.c_uint32)), ("val", C.POINTER(C.c_uint8))]


_P8, _PCSR, _PH, _PI32 = C.POINTER(C.c_uint8), C.POINTER(CSR), C.POINTER(C.c_uint64), C.POINTER(C.c_int32)
_KEYGEN = [C.c_uint32, C.c_uint32, _PCSR, _PCSR, _PCSR, _P8, _P8, C.c_uint32, _P8, C.c_size_t, _P8, C.c_size_t, _P8, _P8, _PH]
# argument types of the key-generation entries, in the header's order (tests/test_keygen_surface.py holds them to include/zkmi355x.h); ctypes then checks
# every call against them.  The older entries are called with explicitly typed ctypes values.
PROTOTYPES = {
    "zk_fr_lagrange_at": [C.c_uint32, C.c_uint32, _P8, _P8, _P8],
    "zk_groth16_keygen": _KEYGEN,
    "zk_pinocchio_keygen": _KEYGEN,
    "zk_pinocchio_pk_upload_lagrange": [C.c_uint32, C.c_uint32, _PCSR, _PCSR, _PCSR, _P8, _P8, C.c_size_t, _P8, C.c_size_t, _P8, _PH],
}
# the batched verifiers and the Fp12 hook, typed the same way (tests/test_verify_many_surface.py holds them to the header).  A table of their own:
# tests/test_keygen_surface.py holds PROTOTYPES to exactly the key-generation entries.
VERIFY_PROTOTYPES = {
    "zk_pairing_product_many": [_P8, _P8, _PH, C.c_uint32, _P8],
    "zk_groth16_verify_many": [_P8, _P8, C.c_size_t, _P8, _P8, _P8, _P8, C.c_uint32, _P8, _PI32],
    "zk_pinocchio_verify_many": [_P8, _P8, C.c_size_t, _P8, _P8, C.c_uint32, _P8, _PI32],
    "zk_selftest_fp12": [C.c_int, _P8, _P8, C.c_size_t, _P8],
}
# the resident verification keys and the subgroup hook (tests/test_verify_resident_surface.py holds them to the header).  Again a table of their own:
# tests/test_verify_many_surface.py holds VERIFY_PROTOTYPES to exactly the batched verifiers.
VK_PROTOTYPES = {
    "zk_groth16_vk_upload": [_P8, _P8, C.c_size_t, _P8, _P8, _PH],
    "zk_pinocchio_vk_upload": [_P8, _P8, C.c_size_t, _PH],
    "zk_vk_info": [C.c_uint64, C.POINTER(C.c_int), _PH],
    "zk_vk_free": [C.c_uint64],
    "zk_groth16_verify_resident": [C.c_uint64, _P8, _P8, C.c_uint32, _P8, _PI32],
    "zk_pinocchio_verify_resident": [C.c_uint64, _P8, _P8, C.c_uint32, _P8, _PI32],
    "zk_selftest_subgroup": [C.c_int, C.c_int, _P8, C.c_size_t, _P8],
}
# the folded verifier and its hook (tests/test_verify_folded_surface.py holds them to the header).  Again a table of their own:
# tests/test_verify_resident_surface.py holds VK_PROTOTYPES to exactly the resident keys' entries.
FOLD_PROTOTYPES = {
    "zk_groth16_verify_folded": [C.c_uint64, _P8, _P8, _P8, C.c_uint32, C.POINTER(C.c_int), _PI32],
    "zk_selftest_groth16_fold": [C.c_uint64, _P8, _P8, _P8, C.c_uint32, _P8, _P8, _P8, _P8, _PI32],
}
# Pinocchio's folded verifier and its hook (tests/test_pinocchio_fold_surface.py holds them to the header).  Again a table of their own:
# tests/test_verify_folded_surface.py holds FOLD_PROTOTYPES to exactly the Groth16 pair.
PIN_FOLD_PROTOTYPES = {
    "zk_pinocchio_verify_folded": [C.c_uint64, _P8, _P8, _P8, C.c_uint32, C.POINTER(C.c_int), _PI32],
    "zk_selftest_pinocchio_fold": [C.c_uint64, _P8, _P8, _P8, C.c_uint32, _P8, _P8, _P8, _PI32],
}
# the same verifiers on proofs in their compressed wire form and the decompression hook (tests/test_verify_compressed_surface.py holds them to the
# header).  Again a table of their own: the tables above are each held to exactly their entries.
COMPRESSED_PROTOTYPES = {
    "zk_groth16_verify_resident_compressed": [C.c_uint64, _P8, _P8, C.c_uint32, _P8, _PI32],
    "zk_pinocchio_verify_resident_compressed": [C.c_uint64, _P8, _P8, C.c_uint32, _P8, _PI32],
    "zk_groth16_verify_folded_compressed": [C.c_uint64, _P8, _P8, _P8, C.c_uint32, C.POINTER(C.c_int), _PI32],
    "zk_pinocchio_verify_folded_compressed": [C.c_uint64, _P8, _P8, _P8, C.c_uint32, C.POINTER(C.c_int), _PI32],
    "zk_selftest_point_decompress": [C.c_int, _P8, C.c_size_t, _P8, _P8],
}
# the group law's hook (tests/test_group_law_surface.py holds it to the header).  Again a table of its own.
GROUP_PROTOTYPES = {
    "zk_selftest_group": [C.c_int, C.c_int, C.c_int, _P8, _P8, C.c_size_t, _P8],
}
# the paired field products' hook (tests/test_gpu_fp_paired.py)
FP_PAIR_PROTOTYPES = {
    "zk_selftest_fp_paired": [C.POINTER(C.c_uint32), C.c_size_t, _P8],
    "zk_selftest_fp2_lanewise": [C.POINTER(C.c_uint32), C.c_size_t, _P8],
}
# the scalar field's hooks (tests/test_fr_selftest_surface.py holds them to the header)
FR_PROTOTYPES = {
    "zk_selftest_fr": [C.c_int, _P8, _P8, C.c_size_t, _P8],
    "zk_selftest_fr29": [C.c_int, C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(C.c_uint32)],
}
# the base field's raw-limb hook (tests/test_fp29_selftest_surface.py holds it to the header).  A table of its own:
# tests/test_fr_selftest_surface.py holds FR_PROTOTYPES to exactly its two entries.
FP29_PROTOTYPES = {
    "zk_selftest_fp29": [C.c_int, C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(C.c_uint32)],
}
# keys and base lists in wire form (tests/test_key_wire_surface.py holds them to the header)
_PSZ = C.POINTER(C.c_size_t)
KEY_WIRE_PROTOTYPES = {
    "zk_groth16_pk_upload_compressed": [C.c_uint32, C.c_uint32, _PCSR, _PCSR, _PCSR, _P8, _P8, C.c_size_t, _P8, C.c_size_t, C.c_uint32, _PH],
    "zk_pinocchio_pk_upload_compressed": [C.c_uint32, C.c_uint32, _PCSR, _PCSR, _PCSR, _P8, _P8, C.c_size_t, _P8, C.c_size_t, _P8, _PH],
    "zk_bases_upload_compressed": [C.c_int, _P8, C.c_size_t, _PH],
    "zk_groth16_pool_points_compressed": [C.c_uint64, C.c_int, _P8, C.c_size_t, _PSZ],
    "zk_pinocchio_pool_points_compressed": [C.c_uint64, C.c_int, _P8, C.c_size_t, _PSZ],
}
# a batch of proofs in one call, out as wire bytes, and the conversion's hook (tests/test_prove_many_surface.py holds them to the header)
PROVE_MANY_PROTOTYPES = {
    "zk_groth16_prove_many_compressed": [C.c_uint64, _P8, _P8, C.c_uint32, C.c_uint32, _P8, _PI32],
    "zk_pinocchio_prove_many_compressed": [C.c_uint64, _P8, _P8, C.c_uint32, C.c_uint32, _P8, _PI32],
    "zk_selftest_proof_wire": [C.c_int, _P8, _P8, C.c_size_t, _P8],
}
# the key check (tests/test_key_check_surface.py holds it to the header)
KEY_CHECK_PROTOTYPES = {
    "zk_groth16_key_check": [C.c_uint64, _P8, C.c_size_t, _P8, _P8, C.POINTER(C.c_uint32)],
}
# the same check of a Lagrange-form handle (tests/test_key_check_lagrange_surface.py holds it to the header).  A table of its own:
# tests/test_key_check_surface.py holds KEY_CHECK_PROTOTYPES to exactly the one entry.
KEY_CHECK_LAGRANGE_PROTOTYPES = {
    "zk_groth16_key_check_lagrange": [C.c_uint64, _P8, C.c_size_t, _P8, _P8, C.POINTER(C.c_uint32)],
}
# the delta contribution and its kernel's hook (tests/test_contribute_surface.py holds them to the header)
CONTRIBUTE_PROTOTYPES = {
    "zk_groth16_pk_contribute": [C.c_uint64, _P8, _P8, _P8, _P8],
    "zk_selftest_g1_scale": [_P8, C.c_size_t, _P8, C.c_uint32, _P8],
}
# a phase-1 string specialised to a circuit, and the hook of its column sums (tests/test_specialize_surface.py holds them to the header)
SPECIALIZE_PROTOTYPES = {
    "zk_groth16_srs_sizes": [C.c_uint32, _PH, _PH, _PH],
    "zk_groth16_pk_specialize": [C.c_uint32, C.c_uint32, _PCSR, _PCSR, _PCSR, _P8, _P8, C.c_size_t, _P8, C.c_size_t, C.c_uint32,
                                 _P8, C.c_size_t, _P8, C.c_size_t, _P8, _P8, _PH],
    "zk_selftest_g1_colsum": [_P8, C.c_size_t, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), _P8, C.c_uint32, _P8],
}
# a phase-1 string checked as a whole and contributed to (tests/test_srs_surface.py holds them to the header).  A table of their own:
# tests/test_specialize_surface.py holds SPECIALIZE_PROTOTYPES to exactly its three entries.
SRS_PROTOTYPES = {
    "zk_groth16_srs_check": [_P8, C.c_size_t, C.c_size_t, _P8, C.c_size_t, _P8, C.POINTER(C.c_uint32)],
    "zk_groth16_srs_contribute": [_P8, C.c_size_t, C.c_size_t, _P8, C.c_size_t, _P8, _P8, _P8, _P8, _P8],
}
# the bits of zk_groth16_srs_check's mask (ZK_SRSCHK_*), in bit order, under the names SRS.check reports
SRSCHK_BITS = {
    "generators": 1, "tau_g1": 2, "tau_g2": 4, "alpha": 8, "beta": 16, "trivial": 32,
}
# the bits of zk_groth16_key_check's mask (ZK_KEYCHK_*), in bit order, under the names Groth16.check_key reports
KEYCHK_BITS = {
    "generators": 1, "tau_g1": 2, "tau_g2": 4, "beta": 8, "delta": 16, "h_bases": 32, "l": 64, "gamma": 128,
}
KEYCHK_AB = 1 << 31          # wrapper-only: vkey.ab is not e(a, b2) (the C call never sees ab: its bytes are the caller's pairing)
KEY_FORMS = {"tau_powers": 0, "lagrange": 1}         # ZK_KEY_FORM_TAU_POWERS, ZK_KEY_FORM_LAGRANGE

_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "%s is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). There is no CPU fallback." % LIB_PATH)
        _lib = C.CDLL(LIB_PATH)
        _lib.zk_strerror.restype = C.c_char_p
        _lib.zk_last_error.restype = C.c_char_p
        for name, args in list(PROTOTYPES.items()) + list(VERIFY_PROTOTYPES.items()) + list(VK_PROTOTYPES.items()) + list(FOLD_PROTOTYPES.items()) + list(PIN_FOLD_PROTOTYPES.items()) + list(COMPRESSED_PROTOTYPES.items()) + list(GROUP_PROTOTYPES.items()) + list(FP_PAIR_PROTOTYPES.items()) + list(FR_PROTOTYPES.items()) + list(FP29_PROTOTYPES.items()) + list(KEY_WIRE_PROTOTYPES.items()) + list(PROVE_MANY_PROTOTYPES.items()) + list(KEY_CHECK_PROTOTYPES.items()) + list(KEY_CHECK_LAGRANGE_PROTOTYPES.items()) + list(CONTRIBUTE_PROTOTYPES.items()) + list(SPECIALIZE_PROTOTYPES.items()) + list(SRS_PROTOTYPES.items()):
            fn = getattr(_lib, name, None)          # absent from the host-only sanitizer build (ZK_LIBZKMI355X_PATH); calling a missing entry still raises
            if fn is not None:
                fn.argtypes, fn.restype = args, C.c_int
    return _lib


def check(rc):
    if rc != 0:
        L = lib()
        raise ZkError(rc, "%s -- %s" % (L.zk_strerror(rc).decode(), L.zk_last_error().decode()))
    return rc


def check_points(rc):
    """check() for the calls that take points in wire form: a point the device decoder refuses (ZK_ERR_ARG, ZK_ERR_NOT_ON_CURVE) raises the ValueError
    of the JSON readers (wire._point_error), with the library's code and text."""
    if rc in (-1, -2):
        from .wire import _point_error
        try:
            check(rc)
        except ZkError as e:
            raise _point_error(e) from None
    return check(rc)


def set_device_list(devices):
    """zk_set_device_list: the devices a key uploaded from now on is sharded over, behind ONE handle (include/zkmi355x.h, "multi-device keys").
    An index may repeat (several shards on one card).  Every key handle must have been freed."""
    arr = (C.c_int32 * len(devices))(*[int(d) for d in devices])
    check(lib().zk_set_device_list(arr, C.c_uint32(len(devices))))


def device_list():
    n = C.c_uint32()
    check(lib().zk_get_device_list(None, C.c_uint32(0), C.byref(n)))
    arr = (C.c_int32 * max(1, n.value))()
    check(lib().zk_get_device_list(arr, C.c_uint32(n.value), C.byref(n)))
    return [int(arr[i]) for i in range(n.value)]


def u8(buf):
    """numpy uint8 array / bytes -> (pointer, keepalive)."""
    import numpy as np
    if isinstance(buf, (bytes, bytearray)):
        arr = np.frombuffer(bytes(buf), dtype=np.uint8)
    else:
        arr = np.ascontiguousarray(buf, dtype=np.uint8)
    return arr.ctypes.data_as(C.POINTER(C.c_uint8)), arr
