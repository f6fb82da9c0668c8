"""Host-side binding of libcityprover_hip.so (the C ABI in include/cityprover.h).

This is plumbing only: every computation happens in the HIP library. There is no CPU fallback —
constructing a `Prover` without a GPU raises `CityProverError`.

The method names mirror what the reference reaches through plonky2 (`PolynomialBatch::from_values`,
`MerkleTree::new`, `PoseidonHash::{hash_no_pad,two_to_one}`, `fft`/`ifft`/`coset_fft`), see
SURVEY.md §8(a).
"""
import ctypes
import os

import numpy as np

from . import build as _build

P = 0xFFFFFFFF00000001
NTT_INVERSE, NTT_BITREV_OUT, NTT_COSET, NTT_BITREV_IN = 1, 2, 4, 8

_u64p = ctypes.POINTER(ctypes.c_uint64)
_vp = ctypes.c_void_p

# name -> (restype, argtypes); must list every symbol declared in include/cityprover.h
ABI = {
    "cp_abi_version": (ctypes.c_int, []),
    "cp_device_count": (ctypes.c_int, []),
    "cp_fault_inject": (ctypes.c_int, [ctypes.c_int, ctypes.c_long]),
    "cp_ctx_create": (_vp, [ctypes.c_int]),
    "cp_ctx_destroy": (None, [_vp]),
    "cp_ctx_set_lanes": (ctypes.c_int, [_vp, ctypes.c_int]),
    "cp_ctx_set_device_transcript": (ctypes.c_int, [_vp, ctypes.c_int]),
    "cp_ctx_set_option": (ctypes.c_int, [_vp, ctypes.c_char_p, ctypes.c_long]),
    "cp_last_error": (ctypes.c_char_p, [_vp]),
    "cp_dev_alloc": (ctypes.c_int, [_vp, ctypes.c_size_t, ctypes.POINTER(_vp)]),
    "cp_dev_free": (ctypes.c_int, [_vp, _vp]),
    "cp_host_alloc": (ctypes.c_int, [_vp, ctypes.c_size_t, ctypes.POINTER(_vp)]),
    "cp_host_free": (ctypes.c_int, [_vp, _vp]),
    "cp_h2d": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_size_t]),
    "cp_d2h": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_size_t]),
    "cp_d2d": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_size_t]),
    "cp_sync": (ctypes.c_int, [_vp]),
    "cp_event_create": (ctypes.c_int, [_vp, ctypes.POINTER(_vp)]),
    "cp_event_destroy": (ctypes.c_int, [_vp, _vp]),
    "cp_event_record": (ctypes.c_int, [_vp, _vp]),
    "cp_event_elapsed_ms": (ctypes.c_int, [_vp, _vp, _vp, ctypes.POINTER(ctypes.c_float)]),
    "cp_profile_begin": (ctypes.c_int, [_vp]),
    "cp_profile_end": (ctypes.c_int, [_vp, ctypes.c_char_p, ctypes.c_size_t]),
    "cp_ntt_dev": (ctypes.c_int, [_vp, _vp, ctypes.c_int, ctypes.c_size_t, ctypes.c_size_t,
                                  ctypes.c_uint, ctypes.c_uint64]),
    "cp_ntt": (ctypes.c_int, [_vp, _u64p, ctypes.c_int, ctypes.c_size_t, ctypes.c_uint,
                              ctypes.c_uint64]),
    "cp_lde_dev": (ctypes.c_int, [_vp, _vp, ctypes.c_size_t, ctypes.c_int, ctypes.c_int,
                                  ctypes.c_size_t, ctypes.c_uint64, ctypes.c_uint, _vp,
                                  ctypes.c_size_t]),
    "cp_poseidon_permute_dev": (ctypes.c_int, [_vp, _vp, ctypes.c_size_t]),
    "cp_field_mul": (ctypes.c_int, [_vp, _u64p, _u64p, _u64p, ctypes.c_size_t]),
    "cp_field_mul2": (ctypes.c_int, [_vp, _u64p, _u64p, _u64p, _u64p, _u64p, _u64p, ctypes.c_size_t]),
    "cp_field_reduce2": (ctypes.c_int, [_vp, _u64p, _u64p, _u64p, _u64p, _u64p, _u64p, ctypes.c_size_t]),
    "cp_poseidon_permute": (ctypes.c_int, [_vp, _u64p, ctypes.c_size_t]),
    "cp_hash_no_pad": (ctypes.c_int, [_vp, _u64p, ctypes.c_size_t, ctypes.c_size_t, _u64p]),
    "cp_two_to_one": (ctypes.c_int, [_vp, _u64p, _u64p, ctypes.c_size_t, _u64p]),
    "cp_merkle_cols_dev": (ctypes.c_int, [_vp, _vp, ctypes.c_size_t, ctypes.c_size_t,
                                          ctypes.c_size_t, ctypes.c_int, _vp, _vp]),
    "cp_merkle_cap": (ctypes.c_int, [_vp, _u64p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int,
                                     _u64p]),
    "cp_commit_dev": (ctypes.c_int, [_vp, _vp, ctypes.c_size_t, ctypes.c_int, ctypes.c_int,
                                     ctypes.c_int, _vp, _vp, _vp, _vp]),
    "cp_commit_batch_dev": (ctypes.c_int, [_vp, _vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int,
                                           ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, _vp]),
}


class CityProverError(RuntimeError):
    pass


_lib = None


def load_library(build_if_missing=True):
    """dlopen the in-tree HIP library; raises if it is missing (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    so = _build.SO
    if not os.path.exists(so):
        if not build_if_missing:
            raise CityProverError(f"{so} not built; run __graft_entry__.build()")
        _build.build()
    lib = ctypes.CDLL(so)
    for name, (res, args) in ABI.items():
        f = getattr(lib, name)  # AttributeError if the symbol is not exported
        f.restype, f.argtypes = res, args
    _lib = lib
    return lib


def _ptr(a):
    assert isinstance(a, np.ndarray) and a.dtype == np.uint64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(_u64p)


def _as_u64(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.uint64))


class DeviceBuffer:
    """A u64 buffer in HBM owned by a Prover context."""

    def __init__(self, prover, n_elems):
        self.prover, self.n = prover, int(n_elems)
        p = _vp()
        prover._check(prover.lib.cp_dev_alloc(prover.ctx, self.n * 8, ctypes.byref(p)))
        self.ptr = p.value

    def upload(self, arr):
        arr = _as_u64(arr)
        assert arr.size <= self.n
        self.prover._check(self.prover.lib.cp_h2d(self.prover.ctx, self.ptr, arr.ctypes.data, arr.size * 8))
        return self

    def download(self, n=None, offset=0):
        n = self.n - offset if n is None else int(n)
        out = np.empty(n, np.uint64)
        self.prover._check(self.prover.lib.cp_d2h(self.prover.ctx, out.ctypes.data, self.ptr + offset * 8, n * 8))
        return out

    def at(self, offset):
        return self.ptr + offset * 8

    @classmethod
    def view(cls, prover, ptr, n_elems):
        """n_elems u64 at a device address that somebody else owns (a key's array): download / at work, free does nothing"""
        self = cls.__new__(cls)
        self.prover, self.n, self.ptr, self.borrowed = prover, int(n_elems), ptr, True
        return self

    def free(self):
        if self.ptr and not getattr(self, "borrowed", False):
            self.prover._check(self.prover.lib.cp_dev_free(self.prover.ctx, self.ptr))
        self.ptr = None


class Prover:
    """One context per GPU (one consumer per device)."""

    def __init__(self, device=0):
        self.lib = load_library()
        if self.lib.cp_device_count() <= 0:
            raise CityProverError("no HIP device visible: cityprover has no CPU fallback")
        self.ctx = self.lib.cp_ctx_create(device)
        if not self.ctx:
            raise CityProverError(self.lib.cp_last_error(None).decode())
        self.device = device

    def close(self):
        if getattr(self, "ctx", None):
            self.free_pinned()
            self.lib.cp_ctx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise CityProverError(f"[{rc}] " + self.lib.cp_last_error(self.ctx).decode())

    # ---- memory / timing -----------------------------------------------------------------
    def alloc(self, n_elems):
        return DeviceBuffer(self, n_elems)

    def set_lanes(self, lanes):
        """internal pipelining of cp_prove_batch_host for a single-threaded caller (cp_ctx_set_lanes)"""
        self._check(self.lib.cp_ctx_set_lanes(self.ctx, int(lanes)))

    def set_option(self, name, value):
        """cp_ctx_set_option: one of the CITYPROVER_* switches for this context only"""
        self._check(self.lib.cp_ctx_set_option(self.ctx, name.encode(), int(value)))

    def set_device_transcript(self, mode):
        """where the Fiat-Shamir transcripts are hashed: 1 device, 0 host, -1 by batch size (cp_ctx_set_device_transcript)"""
        self._check(self.lib.cp_ctx_set_device_transcript(self.ctx, int(mode)))

    def to_device(self, arr):
        arr = _as_u64(arr)
        return DeviceBuffer(self, arr.size).upload(arr)

    def pinned(self, arr):
        """Copy of `arr` (uint64) in page-locked host memory (cp_host_alloc); freed with the Prover or free_pinned()."""
        arr = _as_u64(arr)
        p = _vp()
        self._check(self.lib.cp_host_alloc(self.ctx, arr.size * 8, ctypes.byref(p)))
        out = np.ctypeslib.as_array(ctypes.cast(p, _u64p), shape=(arr.size,)).reshape(arr.shape)
        out[...] = arr
        self._pinned = getattr(self, "_pinned", [])
        self._pinned.append(p.value)
        return out

    def free_pinned(self):
        for p in getattr(self, "_pinned", []):
            self.lib.cp_host_free(self.ctx, p)
        self._pinned = []

    def sync(self):
        self._check(self.lib.cp_sync(self.ctx))

    def event(self):
        e = _vp()
        self._check(self.lib.cp_event_create(self.ctx, ctypes.byref(e)))
        return e.value

    def record(self, ev):
        self._check(self.lib.cp_event_record(self.ctx, ev))

    def elapsed_ms(self, e0, e1):
        ms = ctypes.c_float()
        self._check(self.lib.cp_event_elapsed_ms(self.ctx, e0, e1, ctypes.byref(ms)))
        return ms.value

    def profile_begin(self):
        self._check(self.lib.cp_profile_begin(self.ctx))

    def profile_end(self):
        import json
        buf = ctypes.create_string_buffer(1 << 16)
        self._check(self.lib.cp_profile_end(self.ctx, buf, len(buf)))
        return json.loads(buf.value.decode())

    # ---- device-resident entry points ----------------------------------------------------
    def ntt_dev(self, buf_ptr, log_n, batch=1, stride=None, flags=0, shift=0):
        stride = (1 << log_n) if stride is None else stride
        self._check(self.lib.cp_ntt_dev(self.ctx, buf_ptr, log_n, batch, stride, flags, shift))

    def lde_dev(self, coeffs_ptr, log_n, rate_bits, batch, out_ptr, shift=7, flags=NTT_BITREV_OUT,
                in_stride=None, out_stride=None):
        n = 1 << log_n
        self._check(self.lib.cp_lde_dev(self.ctx, coeffs_ptr, in_stride or n, log_n, rate_bits, batch,
                                        shift, flags, out_ptr, out_stride or (n << rate_bits)))

    def poseidon_permute_dev(self, states_ptr, count):
        self._check(self.lib.cp_poseidon_permute_dev(self.ctx, states_ptr, count))

    def merkle_cols_dev(self, cols_ptr, n_leaves, leaf_len, cap_height, cap_ptr, digests_ptr=None,
                        col_stride=None):
        self._check(self.lib.cp_merkle_cols_dev(self.ctx, cols_ptr, n_leaves, leaf_len,
                                                col_stride or n_leaves, cap_height, digests_ptr, cap_ptr))

    def commit_dev(self, values_ptr, k, log_n, rate_bits, cap_height, lde_ptr, cap_ptr,
                   coeffs_ptr=None, digests_ptr=None):
        self._check(self.lib.cp_commit_dev(self.ctx, values_ptr, k, log_n, rate_bits, cap_height,
                                           coeffs_ptr, lde_ptr, digests_ptr, cap_ptr))

    def commit_batch_dev(self, values_ptr, k, n_trees, log_n, rate_bits, cap_height, lde_ptr, caps_ptr,
                         coeffs_ptr=None, digests_ptr=None):
        self._check(self.lib.cp_commit_batch_dev(self.ctx, values_ptr, k, n_trees, log_n, rate_bits,
                                                 cap_height, coeffs_ptr, lde_ptr, digests_ptr, caps_ptr))

    # ---- host-array conveniences (numpy in / numpy out) -----------------------------------
    def ntt(self, a, flags=0, shift=0):
        a = _as_u64(a).copy()
        batch = 1 if a.ndim == 1 else a.shape[0]
        n = a.shape[-1]
        log_n = int(n).bit_length() - 1
        assert 1 << log_n == n
        self._check(self.lib.cp_ntt(self.ctx, _ptr(a), log_n, batch, flags, shift))
        return a

    def intt(self, a, flags=0, shift=0):
        return self.ntt(a, flags | NTT_INVERSE, shift)

    def lde(self, coeffs, rate_bits, shift=7, bitrev=False):
        c = _as_u64(coeffs)
        c2 = c.reshape(1, -1) if c.ndim == 1 else c
        k, n = c2.shape
        log_n = int(n).bit_length() - 1
        din, dout = self.to_device(c2), self.alloc(k * (n << rate_bits))
        try:
            self.lde_dev(din.ptr, log_n, rate_bits, k, dout.ptr, shift, NTT_BITREV_OUT if bitrev else 0)
            out = dout.download().reshape(k, n << rate_bits)
        finally:
            din.free()
            dout.free()
        return out[0] if c.ndim == 1 else out

    def field_mul(self, a, b):
        """a * b mod p element-wise with the device's multiplication; a, b: any u64 (lazy representatives allowed)."""
        x, y = _as_u64(a).ravel().copy(), _as_u64(b).ravel().copy()
        assert x.size == y.size
        out = np.zeros(x.size, np.uint64)
        self._check(self.lib.cp_field_mul(self.ctx, _ptr(x), _ptr(y), _ptr(out), x.size))
        return out

    def field_mul2(self, a, b, c, d):
        """(a * b, c * d) mod p element-wise with the device's paired product (one lane computes both); any u64 in."""
        v = [_as_u64(x).ravel().copy() for x in (a, b, c, d)]
        assert all(x.size == v[0].size for x in v)
        out_ab, out_cd = np.zeros(v[0].size, np.uint64), np.zeros(v[0].size, np.uint64)
        self._check(self.lib.cp_field_mul2(self.ctx, _ptr(v[0]), _ptr(v[1]), _ptr(v[2]), _ptr(v[3]), _ptr(out_ab), _ptr(out_cd), v[0].size))
        return out_ab, out_cd

    def field_reduce2(self, lo_a, hi_a, lo_b, hi_b):
        """(lo_a + hi_a 2^64, lo_b + hi_b 2^64) mod p element-wise with the device's paired reduction (one lane reduces both); any words in."""
        v = [_as_u64(x).ravel().copy() for x in (lo_a, hi_a, lo_b, hi_b)]
        assert all(x.size == v[0].size for x in v)
        out_a, out_b = np.zeros(v[0].size, np.uint64), np.zeros(v[0].size, np.uint64)
        self._check(self.lib.cp_field_reduce2(self.ctx, _ptr(v[0]), _ptr(v[1]), _ptr(v[2]), _ptr(v[3]), _ptr(out_a), _ptr(out_b), v[0].size))
        return out_a, out_b

    def poseidon_permute(self, states):
        s = _as_u64(states).copy()
        assert s.size % 12 == 0
        self._check(self.lib.cp_poseidon_permute(self.ctx, _ptr(s), s.size // 12))
        return s

    def hash_no_pad(self, inputs):
        x = _as_u64(inputs)
        x2 = x.reshape(1, -1) if x.ndim == 1 else x
        out = np.zeros((x2.shape[0], 4), np.uint64)
        self._check(self.lib.cp_hash_no_pad(self.ctx, _ptr(x2), x2.shape[0], x2.shape[1], _ptr(out)))
        return out[0] if x.ndim == 1 else out

    def two_to_one(self, left, right):
        l, r = _as_u64(left), _as_u64(right)
        l2, r2 = l.reshape(-1, 4), r.reshape(-1, 4)
        out = np.zeros_like(l2)
        self._check(self.lib.cp_two_to_one(self.ctx, _ptr(l2), _ptr(r2), l2.shape[0], _ptr(out)))
        return out.reshape(l.shape)

    def merkle_cap(self, rows, cap_height):
        rows = _as_u64(rows)
        n, k = rows.shape
        cap = np.zeros((1 << cap_height, 4), np.uint64)
        self._check(self.lib.cp_merkle_cap(self.ctx, _ptr(rows), n, k, cap_height, _ptr(cap)))
        return cap

    def merkle_cols(self, cols, cap_height, want_digests=False):
        cols = _as_u64(cols)
        k, n = cols.shape
        dc, dcap = self.to_device(cols), self.alloc(4 << cap_height)
        nd = 2 * n - (2 << cap_height)
        dd = self.alloc(nd * 4) if want_digests and nd > 0 else None
        try:
            self.merkle_cols_dev(dc.ptr, n, k, cap_height, dcap.ptr, dd.ptr if dd else None)
            cap = dcap.download().reshape(-1, 4)
            dig = dd.download().reshape(-1, 4) if dd else None
        finally:
            dc.free()
            dcap.free()
            if dd:
                dd.free()
        return (cap, dig) if want_digests else cap

    def commit(self, values, rate_bits, cap_height, want=("coeffs", "lde", "cap")):
        v = _as_u64(values)
        k, n = v.shape
        log_n = int(n).bit_length() - 1
        N = n << rate_bits
        dv, dl, dcap = self.to_device(v), self.alloc(k * N), self.alloc(4 << cap_height)
        dco = self.alloc(k * n) if "coeffs" in want else None
        nd = 2 * N - (2 << cap_height)
        dd = self.alloc(nd * 4) if "digests" in want and nd > 0 else None
        try:
            self.commit_dev(dv.ptr, k, log_n, rate_bits, cap_height, dl.ptr, dcap.ptr,
                            dco.ptr if dco else None, dd.ptr if dd else None)
            res = {"cap": dcap.download().reshape(-1, 4)}
            res["lde"] = dl.download().reshape(k, N) if "lde" in want else None
            res["coeffs"] = dco.download().reshape(k, n) if dco else None
            res["digests"] = dd.download().reshape(-1, 4) if dd else None
        finally:
            for b in (dv, dl, dcap, dco, dd):
                if b:
                    b.free()
        return res


# ---- circuits and the proof tail ---------------------------------------------------------------
class Shape(ctypes.Structure):
    """cp_shape (include/cityprover.h)."""
    _fields_ = [(n, ctypes.c_int) for n in (
        "degree_bits", "num_constants", "num_routed_wires", "num_wires", "num_challenges",
        "num_partial_products", "quotient_degree_factor", "rate_bits", "cap_height", "pow_bits",
        "num_query_rounds", "n_arity")] + [("arity_bits", ctypes.c_int * 8), ("zero_knowledge", ctypes.c_int),
                                            ("num_public_inputs", ctypes.c_int)]


SALT_SIZE = 4


def standard_recursion_shape(**over):
    """CircuitConfig::standard_recursion_config() at degree 2^12, the only configuration the worker
    circuits use (SURVEY.md §5 'Config / flags', Appendix A)."""
    d = dict(degree_bits=12, num_constants=5, num_routed_wires=80, num_wires=135, num_challenges=2,
             num_partial_products=9, quotient_degree_factor=8, rate_bits=3, cap_height=4, pow_bits=16,
             num_query_rounds=28, arity_bits=(4, 4), zero_knowledge=0, num_public_inputs=0)
    d.update(over)
    ab = d.pop("arity_bits")
    s = Shape(**d, n_arity=len(ab))
    for i, a in enumerate(ab):
        s.arity_bits[i] = a
    return s


ABI.update({
    "cp_circuit_load": (_vp, [_vp, ctypes.POINTER(Shape), _u64p, _u64p, _u64p]),
    "cp_zs_partial_products_dev": (ctypes.c_int, [_vp, ctypes.c_size_t, ctypes.POINTER(_vp), _vp, _u64p, _u64p, _vp]),
    "cp_circuit_destroy": (None, [_vp]),
    "cp_circuit_cs_cap": (ctypes.c_int, [_vp, _u64p]),
    "cp_circuits_batch_compatible": (ctypes.c_int, [_vp, _vp]),
    "cp_prove_tail": (ctypes.c_int, [_vp, _u64p, ctypes.c_size_t, _vp, _vp, _vp, ctypes.c_int, ctypes.c_uint64,
                                     ctypes.POINTER(ctypes.POINTER(ctypes.c_uint8)),
                                     ctypes.POINTER(ctypes.c_size_t)]),
    "cp_free": (None, [_vp]),
})


class Circuit:
    """Device-resident circuit: the mirror of a built `CircuitData` (constants/sigmas commitment)."""

    def __init__(self, prover, shape, circuit_digest, cs_values, k_is=None):
        self.prover, self.shape = prover, shape
        cd, cs = _as_u64(circuit_digest), _as_u64(cs_values)
        n = 1 << shape.degree_bits
        assert cs.shape == (shape.num_constants + shape.num_routed_wires, n)
        ks = None if k_is is None else _as_u64(k_is)
        self.handle = prover.lib.cp_circuit_load(prover.ctx, ctypes.byref(shape), _ptr(cd), _ptr(cs),
                                                 None if ks is None else _ptr(ks))
        if not self.handle:
            raise CityProverError(prover.lib.cp_last_error(prover.ctx).decode())

    def cs_cap(self):
        cap = np.zeros((1 << self.shape.cap_height, 4), np.uint64)
        self.prover._check(self.prover.lib.cp_circuit_cs_cap(self.handle, _ptr(cap)))
        return cap

    def prove_tail(self, public_inputs, wires_values, zs_pp_values, quotient_coeffs, pow_override=None):
        """numpy in (uploaded here), bincode ProofWithPublicInputs bytes out."""
        p = self.prover
        pi = _as_u64(public_inputs)
        bufs = [p.to_device(_as_u64(a)) for a in (wires_values, zs_pp_values, quotient_coeffs)]
        try:
            return self.prove_tail_dev(pi, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, pow_override)
        finally:
            for b in bufs:
                b.free()

    def prove_tail_dev(self, public_inputs, wires_ptr, zs_pp_ptr, quotient_ptr, pow_override=None):
        p = self.prover
        pi = _as_u64(public_inputs)
        out = ctypes.POINTER(ctypes.c_uint8)()
        ln = ctypes.c_size_t()
        p._check(p.lib.cp_prove_tail(self.handle, _ptr(pi) if pi.size else None, pi.size, wires_ptr, zs_pp_ptr,
                                     quotient_ptr, 0 if pow_override is None else 1, pow_override or 0,
                                     ctypes.byref(out), ctypes.byref(ln)))
        data = ctypes.string_at(out, ln.value)
        p.lib.cp_free(out)
        return data

    def close(self):
        if self.handle:
            self.prover.lib.cp_circuit_destroy(self.handle)
            self.handle = None


ABI["cp_prove_tail_batch"] = (ctypes.c_int, [_vp, ctypes.c_size_t, ctypes.POINTER(_vp), ctypes.POINTER(_u64p),
                                             ctypes.POINTER(ctypes.c_size_t), _vp, _vp, _vp,
                                             ctypes.POINTER(ctypes.c_int), _u64p,
                                             ctypes.POINTER(ctypes.POINTER(ctypes.c_uint8)),
                                             ctypes.POINTER(ctypes.c_size_t)])


def prove_tail_batch_dev(prover, circuits, public_inputs, wires_ptr, zs_pp_ptr, quotient_ptr, pow_overrides=None):
    """circuits: list of Circuit (same shape); public_inputs: list of u64 sequences; device pointers hold
    [proof][poly][n]. Returns a list of proof byte strings."""
    B = len(circuits)
    cs = (_vp * B)(*[c.handle for c in circuits])
    pis = [_as_u64(p) for p in public_inputs]
    pi_ptrs = (_u64p * B)(*[_ptr(p) if p.size else None for p in pis])
    n_pis = (ctypes.c_size_t * B)(*[p.size for p in pis])
    use = (ctypes.c_int * B)(*[0 if (pow_overrides is None or pow_overrides[i] is None) else 1 for i in range(B)])
    ov = np.array([0 if (pow_overrides is None or pow_overrides[i] is None) else pow_overrides[i] for i in range(B)],
                  dtype=np.uint64)
    outs = (ctypes.POINTER(ctypes.c_uint8) * B)()
    lens = (ctypes.c_size_t * B)()
    prover._check(prover.lib.cp_prove_tail_batch(prover.ctx, B, cs, pi_ptrs, n_pis, wires_ptr, zs_pp_ptr, quotient_ptr,
                                                 use, _ptr(ov), outs, lens))
    res = []
    for i in range(B):
        res.append(ctypes.string_at(outs[i], lens[i]))
        prover.lib.cp_free(outs[i])
    return res


def zs_partial_products_dev(prover, circuits, wires_ptr, betas, gammas, out_ptr):
    """A7 for a batch: betas/gammas are (B, num_challenges) arrays; device buffers as in the header."""
    B = len(circuits)
    cs = (_vp * B)(*[c.handle for c in circuits])
    b, g = _as_u64(betas).reshape(B, -1), _as_u64(gammas).reshape(B, -1)
    prover._check(prover.lib.cp_zs_partial_products_dev(prover.ctx, B, cs, wires_ptr, _ptr(b), _ptr(g), out_ptr))


# ---- gates and the whole proof ------------------------------------------------------------------------
GATE_NOOP, GATE_CONSTANT, GATE_PUBLIC_INPUT, GATE_ARITHMETIC, GATE_POSEIDON = 0, 1, 2, 3, 4
GATE_COMPARISON, GATE_U32_ARITHMETIC, GATE_U32_RANGE_CHECK = 5, 6, 7
GATE_U32_ADD_MANY, GATE_U32_SUBTRACTION, GATE_U32_INTERLEAVE, GATE_UNINTERLEAVE_TO_U32, GATE_UNINTERLEAVE_TO_B32 = 8, 9, 10, 11, 12
(GATE_ARITHMETIC_EXT, GATE_MUL_EXT, GATE_BASE_SUM, GATE_RANDOM_ACCESS, GATE_REDUCING, GATE_REDUCING_EXT, GATE_POSEIDON_MDS,
 GATE_COSET_INTERPOLATION) = 13, 14, 15, 16, 17, 18, 19, 20
GATE_EXPONENTIATION = 21


class Gate(ctypes.Structure):
    """cp_gate"""
    _fields_ = [(n, ctypes.c_int) for n in ("type", "selector_index", "group_start", "group_end", "param", "param2", "param3")]


ABI["cp_circuit_set_gates"] = (ctypes.c_int, [_vp, ctypes.POINTER(Gate), ctypes.c_size_t, ctypes.c_int])
ABI["cp_prove_batch"] = (ctypes.c_int, [_vp, ctypes.c_size_t, ctypes.POINTER(_vp), ctypes.POINTER(_u64p),
                                        ctypes.POINTER(ctypes.c_size_t), _vp, ctypes.POINTER(ctypes.c_int), _u64p,
                                        ctypes.POINTER(ctypes.POINTER(ctypes.c_uint8)),
                                        ctypes.POINTER(ctypes.c_size_t)])


def set_gates(circuit, gate_list, num_selectors):
    """gate_list: [(type, selector_index, group_start, group_end, param[, param2[, param3]])] in gate-index order."""
    arr = (Gate * len(gate_list))(*[Gate(*(tuple(g) + (0,) * (7 - len(g)))) for g in gate_list])
    circuit.prover._check(circuit.prover.lib.cp_circuit_set_gates(circuit.handle, arr, len(gate_list), num_selectors))
    circuit.n_gates = len(gate_list)


def prove_batch_dev(prover, circuits, public_inputs, wires_ptr, pow_overrides=None):
    """wires -> proofs for a batch (A7 + A8 + tail). wires_ptr: device [proof][num_wires][n]."""
    B = len(circuits)
    cs = (_vp * B)(*[c.handle for c in circuits])
    pis = [_as_u64(p) for p in public_inputs]
    pi_ptrs = (_u64p * B)(*[_ptr(p) if p.size else None for p in pis])
    n_pis = (ctypes.c_size_t * B)(*[p.size for p in pis])
    use = (ctypes.c_int * B)(*[0 if (pow_overrides is None or pow_overrides[i] is None) else 1 for i in range(B)])
    ov = np.array([0 if (pow_overrides is None or pow_overrides[i] is None) else pow_overrides[i] for i in range(B)],
                  dtype=np.uint64)
    outs = (ctypes.POINTER(ctypes.c_uint8) * B)()
    lens = (ctypes.c_size_t * B)()
    prover._check(prover.lib.cp_prove_batch(prover.ctx, B, cs, pi_ptrs, n_pis, wires_ptr, use, _ptr(ov), outs, lens))
    res = []
    for i in range(B):
        res.append(ctypes.string_at(outs[i], lens[i]))
        prover.lib.cp_free(outs[i])
    return res


ABI["cp_prove_batch_host"] = (ctypes.c_int, [_vp, ctypes.c_size_t, ctypes.POINTER(_vp), ctypes.POINTER(_u64p),
                                             ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(_u64p),
                                             ctypes.POINTER(ctypes.c_int), _u64p,
                                             ctypes.POINTER(ctypes.POINTER(ctypes.c_uint8)),
                                             ctypes.POINTER(ctypes.c_size_t)])
ABI["cp_prove"] = (ctypes.c_int, [_vp, _u64p, _u64p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint64,
                                  ctypes.POINTER(ctypes.POINTER(ctypes.c_uint8)), ctypes.POINTER(ctypes.c_size_t)])


def prove_batch(prover, circuits, public_inputs, wires, pow_overrides=None):
    """Host-memory variant (cp_prove_batch_host): wires = list of [num_wires][n] uint64 arrays (the witness generator's
    output); the library copies them to the device."""
    B = len(circuits)
    cs = (_vp * B)(*[c.handle for c in circuits])
    pis = [_as_u64(p) for p in public_inputs]
    pi_ptrs = (_u64p * B)(*[_ptr(p) if p.size else None for p in pis])
    n_pis = (ctypes.c_size_t * B)(*[p.size for p in pis])
    ws = [_as_u64(w) for w in wires]
    for c, w in zip(circuits, ws):   # the C ABI takes bare pointers: sizes are checked here
        if w.size != c.shape.num_wires << c.shape.degree_bits:
            raise ValueError("wires must be [num_wires][n] = %d x %d values" % (c.shape.num_wires, 1 << c.shape.degree_bits))
    w_ptrs = (_u64p * B)(*[_ptr(w) for w in ws])
    use = (ctypes.c_int * B)(*[0 if (pow_overrides is None or pow_overrides[i] is None) else 1 for i in range(B)])
    ov = np.array([0 if (pow_overrides is None or pow_overrides[i] is None) else pow_overrides[i] for i in range(B)],
                  dtype=np.uint64)
    outs = (ctypes.POINTER(ctypes.c_uint8) * B)()
    lens = (ctypes.c_size_t * B)()
    prover._check(prover.lib.cp_prove_batch_host(prover.ctx, B, cs, pi_ptrs, n_pis, w_ptrs, use, _ptr(ov), outs, lens))
    res = []
    for i in range(B):
        res.append(ctypes.string_at(outs[i], lens[i]))
        prover.lib.cp_free(outs[i])
    return res


ABI["cp_prove_batch_zk_host"] = (ctypes.c_int, [_vp, ctypes.c_size_t, ctypes.POINTER(_vp), ctypes.POINTER(_u64p),
                                                ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(_u64p), ctypes.POINTER(_u64p),
                                                ctypes.POINTER(ctypes.c_int), _u64p,
                                                ctypes.POINTER(ctypes.POINTER(ctypes.c_uint8)),
                                                ctypes.POINTER(ctypes.c_size_t)])


def prove_batch_zk(prover, circuits, public_inputs, wires, salts, pow_overrides=None):
    """Zero-knowledge circuits: salts[p] = [3][SALT_SIZE][N] uint64 random field elements (cp_prove_batch_zk_host)."""
    B = len(circuits)
    cs = (_vp * B)(*[c.handle for c in circuits])
    pis = [_as_u64(p) for p in public_inputs]
    pi_ptrs = (_u64p * B)(*[_ptr(p) if p.size else None for p in pis])
    n_pis = (ctypes.c_size_t * B)(*[p.size for p in pis])
    ws, sl = [_as_u64(w) for w in wires], [_as_u64(x) for x in salts]
    for c, w, x in zip(circuits, ws, sl):   # the C ABI takes bare pointers: sizes are checked here
        if w.size != c.shape.num_wires << c.shape.degree_bits:
            raise ValueError("wires must be [num_wires][n]")
        if x.size != 3 * SALT_SIZE << (c.shape.degree_bits + c.shape.rate_bits):
            raise ValueError("salts must be [3][SALT_SIZE][N]")
    w_ptrs = (_u64p * B)(*[_ptr(w) for w in ws])
    s_ptrs = (_u64p * B)(*[_ptr(x) for x in sl])
    use = (ctypes.c_int * B)(*[0 if (pow_overrides is None or pow_overrides[i] is None) else 1 for i in range(B)])
    ov = np.array([0 if (pow_overrides is None or pow_overrides[i] is None) else pow_overrides[i] for i in range(B)],
                  dtype=np.uint64)
    outs = (ctypes.POINTER(ctypes.c_uint8) * B)()
    lens = (ctypes.c_size_t * B)()
    prover._check(prover.lib.cp_prove_batch_zk_host(prover.ctx, B, cs, pi_ptrs, n_pis, w_ptrs, s_ptrs, use, _ptr(ov), outs, lens))
    res = []
    for i in range(B):
        res.append(ctypes.string_at(outs[i], lens[i]))
        prover.lib.cp_free(outs[i])
    return res


def prove(circuit, wires, public_inputs, pow_override=None):
    """cp_prove: CircuitData::prove after witness generation for ONE proof, wires in host memory."""
    pr = circuit.prover
    w, pi = _as_u64(wires), _as_u64(public_inputs)
    if w.size != circuit.shape.num_wires << circuit.shape.degree_bits:
        raise ValueError("wires must be [num_wires][n]")
    out = ctypes.POINTER(ctypes.c_uint8)()
    n = ctypes.c_size_t()
    pr._check(pr.lib.cp_prove(circuit.handle, _ptr(w), _ptr(pi) if pi.size else None, pi.size,
                              0 if pow_override is None else 1, 0 if pow_override is None else pow_override,
                              ctypes.byref(out), ctypes.byref(n)))
    res = ctypes.string_at(out, n.value)
    pr.lib.cp_free(out)
    return res


class BatcherStats(ctypes.Structure):
    """cp_batcher_stats"""
    _fields_ = [("calls", ctypes.c_uint64), ("batches", ctypes.c_uint64), ("proofs", ctypes.c_uint64),
                ("largest_batch", ctypes.c_uint64), ("retried_singly", ctypes.c_uint64)]


ABI["cp_batcher_create"] = (_vp, [_vp, ctypes.c_size_t, ctypes.c_uint])
ABI["cp_batcher_prove"] = (ctypes.c_int, [_vp, _vp, _u64p, _u64p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint64,
                                          ctypes.POINTER(ctypes.POINTER(ctypes.c_uint8)), ctypes.POINTER(ctypes.c_size_t)])
ABI["cp_batcher_get_stats"] = (ctypes.c_int, [_vp, ctypes.POINTER(BatcherStats)])
ABI["cp_batcher_destroy"] = (None, [_vp])


class Batcher:
    """cp_batcher: merges the concurrent one-proof calls of several threads (the reference's worker loops,
    city_rollup_core_worker/src/actors/simple.rs:32-56) into cp_prove_batch_host launches. `prove` is thread-safe
    and blocking (ctypes releases the GIL for the call)."""

    def __init__(self, prover, max_batch=32, linger_us=0):
        self.prover = prover
        self.handle = prover.lib.cp_batcher_create(prover.ctx, max_batch, linger_us)
        if not self.handle:
            raise CityProverError(prover.lib.cp_last_error(None).decode())

    def prove(self, circuit, wires, public_inputs, pow_override=None):
        lib = self.prover.lib
        w, pi = _as_u64(wires), _as_u64(public_inputs)
        if w.size != circuit.shape.num_wires << circuit.shape.degree_bits:
            raise ValueError("wires must be [num_wires][n]")
        out = ctypes.POINTER(ctypes.c_uint8)()
        n = ctypes.c_size_t()
        rc = lib.cp_batcher_prove(self.handle, circuit.handle, _ptr(w), _ptr(pi) if pi.size else None, pi.size,
                                  0 if pow_override is None else 1, 0 if pow_override is None else pow_override,
                                  ctypes.byref(out), ctypes.byref(n))
        if rc != 0:  # the message is the calling thread's, not the context's
            raise CityProverError(f"[{rc}] " + lib.cp_last_error(None).decode())
        res = ctypes.string_at(out, n.value)
        lib.cp_free(out)
        return res

    def stats(self):
        st = BatcherStats()
        self.prover._check(self.prover.lib.cp_batcher_get_stats(self.handle, ctypes.byref(st)))
        return {k: int(getattr(st, k)) for k, _ in BatcherStats._fields_}

    def close(self):
        if self.handle:
            self.prover.lib.cp_batcher_destroy(self.handle)
            self.handle = None


ABI["cp_verify"] = (ctypes.c_int, [_vp, ctypes.c_char_p, ctypes.c_size_t])


def verify(circuit, proof_bytes):
    """CircuitData::verify. Returns None when the proof is accepted; raises CityProverError naming the
    first failing check otherwise."""
    circuit.prover._check(circuit.prover.lib.cp_verify(circuit.handle, proof_bytes, len(proof_bytes)))


# ---- BLS12-381 G1 MSM -------------------------------------------------------------------
_u8p = ctypes.POINTER(ctypes.c_uint8)
ABI["cp_msm_bls12381_g1"] = (ctypes.c_int, [_vp, _u64p, _u64p, _u8p, ctypes.c_size_t, _u64p, ctypes.POINTER(ctypes.c_int)])
ABI["cp_msm_bls12381_g1_prepare_dev"] = (ctypes.c_int, [_vp, _vp, ctypes.c_size_t, _vp])
ABI["cp_msm_bls12381_g1_dev"] = (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_size_t, _u64p, ctypes.POINTER(ctypes.c_int)])
ABI["cp_msm_bls12381_g1_synthetic_points_dev"] = (ctypes.c_int, [_vp, _u64p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_size_t, _vp])
ABI["cp_fixed_base_mul_bls12381_g1_dev"] = (ctypes.c_int, [_vp, _u64p, _vp, ctypes.c_size_t, _vp, _vp])
G1_AFFINE_BYTES = 112
BLS_P = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab
_BLS_RINV = pow(1 << 392, -1, BLS_P)   # the internal form is Montgomery, radix 2^392, in 14 limbs of 28 bits


def _coords_to_host(buf, n, per_point, index=None):
    """the coordinates of points in the library's internal form as canonical ints: (len(index), per_point)"""
    limbs = buf.download(n * per_point * 7).view(np.uint32).reshape(n, per_point, 14)
    rows = range(n) if index is None else index
    return [[sum(int(l) << (28 * j) for j, l in enumerate(limbs[i, c])) * _BLS_RINV % BLS_P for c in range(per_point)] for i in rows]


def _flags_buffer(prover, n):
    return prover.alloc((n + 7) // 8)


def flags_to_host(buf, n):
    """a device byte-flag array of n entries (in a u64 buffer) as uint8"""
    return buf.download((n + 7) // 8).view(np.uint8)[:n].copy()


def _g1_out(xy, inf):
    if inf.value:
        return None
    return (sum(int(v) << (64 * i) for i, v in enumerate(xy[:6])), sum(int(v) << (64 * i) for i, v in enumerate(xy[6:])))


def msm_g1(prover, scalars, points_xy, points_inf=None):
    """sum_i scalars[i] * points[i] on BLS12-381 G1. scalars: (n, 4) uint64 LE limbs; points_xy: (n, 12) uint64 affine
    canonical x || y; points_inf: optional (n,) uint8. Returns None (infinity) or (x, y) Python ints."""
    s, p = _as_u64(scalars).reshape(-1, 4), _as_u64(points_xy).reshape(-1, 12)
    if s.shape[0] != p.shape[0]:
        raise ValueError("scalars and points differ in count")
    n = s.shape[0]
    inf = None if points_inf is None else np.ascontiguousarray(points_inf, dtype=np.uint8)
    out, oi = np.zeros(12, np.uint64), ctypes.c_int()
    prover._check(prover.lib.cp_msm_bls12381_g1(prover.ctx, _ptr(s) if n else None, _ptr(p) if n else None,
                                                None if inf is None else inf.ctypes.data_as(_u8p), n, _ptr(out),
                                                ctypes.byref(oi)))
    return _g1_out(out, oi)


class G1Points:
    """A fixed point set resident on the device in the library's internal form (a proving key)."""

    def __init__(self, prover, points_xy):
        p = _as_u64(points_xy).reshape(-1, 12)
        self.prover, self.n = prover, p.shape[0]
        raw = prover.to_device(p)
        self.buf = prover.alloc(self.n * G1_AFFINE_BYTES // 8)
        prover._check(prover.lib.cp_msm_bls12381_g1_prepare_dev(prover.ctx, raw.ptr, self.n, self.buf.ptr))
        prover.sync()
        raw.free()

    @classmethod
    def synthetic(cls, prover, generator, a, b, n):
        """P_i = (a*i + b) * generator, built on the device (bench / large tests)."""
        self = cls.__new__(cls)
        self.prover, self.n = prover, n
        self.buf = prover.alloc(n * G1_AFFINE_BYTES // 8)
        g = np.array([(int(generator[h]) >> (64 * i)) & (2**64 - 1) for h in range(2) for i in range(6)], dtype=np.uint64)
        prover._check(prover.lib.cp_msm_bls12381_g1_synthetic_points_dev(prover.ctx, _ptr(g), a, b, n, self.buf.ptr))
        prover.sync()
        return self

    @classmethod
    def fixed_base(cls, prover, base, scalars_ptr, n):
        """(points, flags): points[i] = scalars[i] * base for the n scalars (4 u64 each) at scalars_ptr, built on the device
        (cp_fixed_base_mul_bls12381_g1_dev); flags: a device buffer of n bytes, 1 = the point at infinity. base: (x, y) ints."""
        self = cls.__new__(cls)
        self.prover, self.n = prover, n
        self.buf = prover.alloc(max(n, 1) * G1_AFFINE_BYTES // 8)
        flags = _flags_buffer(prover, max(n, 1))
        g = np.array([(int(base[h]) >> (64 * i)) & (2**64 - 1) for h in range(2) for i in range(6)], dtype=np.uint64)
        try:
            prover._check(prover.lib.cp_fixed_base_mul_bls12381_g1_dev(prover.ctx, _ptr(g), scalars_ptr, n, self.buf.ptr, flags.ptr))
            prover.sync()
        except CityProverError:
            self.buf.free()
            flags.free()
            raise
        return self, flags

    @classmethod
    def view(cls, prover, ptr, n):
        """n points of a set that somebody else owns (a key's)"""
        self = cls.__new__(cls)
        self.prover, self.n, self.buf = prover, n, DeviceBuffer.view(prover, ptr, n * G1_AFFINE_BYTES // 8)
        return self

    def to_host(self, index=None):
        """the points (all, or those at `index`) as (x, y) ints: a test and debugging aid, Python arithmetic per point"""
        return [tuple(c) for c in _coords_to_host(self.buf, self.n, 2, index)]

    def msm_dev(self, scalars_ptr, inf_ptr=None):
        out, oi = np.zeros(12, np.uint64), ctypes.c_int()
        self.prover._check(self.prover.lib.cp_msm_bls12381_g1_dev(self.prover.ctx, scalars_ptr, self.buf.ptr, inf_ptr, self.n,
                                                                  _ptr(out), ctypes.byref(oi)))
        return _g1_out(out, oi)

    def free(self):
        self.buf.free()


# ---- G2 (coordinates c0 + c1*u in F_p^2; a point is 24 uint64: x.c0, x.c1, y.c0, y.c1) ----
ABI["cp_msm_bls12381_g2"] = (ctypes.c_int, [_vp, _u64p, _u64p, _u8p, ctypes.c_size_t, _u64p, ctypes.POINTER(ctypes.c_int)])
ABI["cp_msm_bls12381_g2_prepare_dev"] = (ctypes.c_int, [_vp, _vp, ctypes.c_size_t, _vp])
ABI["cp_msm_bls12381_g2_synthetic_points_dev"] = (ctypes.c_int, [_vp, _u64p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_size_t, _vp])
ABI["cp_msm_bls12381_g2_dev"] = (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_size_t, _u64p, ctypes.POINTER(ctypes.c_int)])
ABI["cp_fixed_base_mul_bls12381_g2_dev"] = (ctypes.c_int, [_vp, _u64p, _vp, ctypes.c_size_t, _vp, _vp])
G2_AFFINE_BYTES = 224


def _g2_out(xy, inf):
    if inf.value:
        return None
    v = [sum(int(x) << (64 * i) for i, x in enumerate(xy[6 * k:6 * k + 6])) for k in range(4)]
    return ((v[0], v[1]), (v[2], v[3]))


def msm_g2(prover, scalars, points_xy, points_inf=None):
    """G2 MSM. points_xy: (n, 24) uint64. Returns None or ((x0, x1), (y0, y1))."""
    s, p = _as_u64(scalars).reshape(-1, 4), _as_u64(points_xy).reshape(-1, 24)
    if s.shape[0] != p.shape[0]:
        raise ValueError("scalars and points differ in count")
    n = s.shape[0]
    inf = None if points_inf is None else np.ascontiguousarray(points_inf, dtype=np.uint8)
    out, oi = np.zeros(24, np.uint64), ctypes.c_int()
    prover._check(prover.lib.cp_msm_bls12381_g2(prover.ctx, _ptr(s) if n else None, _ptr(p) if n else None,
                                                None if inf is None else inf.ctypes.data_as(_u8p), n, _ptr(out),
                                                ctypes.byref(oi)))
    return _g2_out(out, oi)


class G2Points:
    """A fixed G2 point set resident on the device in the library's internal form."""

    def __init__(self, prover, points_xy):
        p = _as_u64(points_xy).reshape(-1, 24)
        self.prover, self.n = prover, p.shape[0]
        raw = prover.to_device(p)
        self.buf = prover.alloc(self.n * G2_AFFINE_BYTES // 8)
        prover._check(prover.lib.cp_msm_bls12381_g2_prepare_dev(prover.ctx, raw.ptr, self.n, self.buf.ptr))
        prover.sync()
        raw.free()

    @classmethod
    def synthetic(cls, prover, generator, a, b, n):
        self = cls.__new__(cls)
        self.prover, self.n = prover, n
        self.buf = prover.alloc(n * G2_AFFINE_BYTES // 8)
        (x0, x1), (y0, y1) = generator
        g = np.array([(int(c) >> (64 * i)) & (2**64 - 1) for c in (x0, x1, y0, y1) for i in range(6)], dtype=np.uint64)
        prover._check(prover.lib.cp_msm_bls12381_g2_synthetic_points_dev(prover.ctx, _ptr(g), a, b, n, self.buf.ptr))
        prover.sync()
        return self

    @classmethod
    def fixed_base(cls, prover, base, scalars_ptr, n):
        """G1Points.fixed_base over G2 (cp_fixed_base_mul_bls12381_g2_dev). base: ((x0, x1), (y0, y1)) ints."""
        self = cls.__new__(cls)
        self.prover, self.n = prover, n
        self.buf = prover.alloc(max(n, 1) * G2_AFFINE_BYTES // 8)
        flags = _flags_buffer(prover, max(n, 1))
        (x0, x1), (y0, y1) = base
        g = np.array([(int(c) >> (64 * i)) & (2**64 - 1) for c in (x0, x1, y0, y1) for i in range(6)], dtype=np.uint64)
        try:
            prover._check(prover.lib.cp_fixed_base_mul_bls12381_g2_dev(prover.ctx, _ptr(g), scalars_ptr, n, self.buf.ptr, flags.ptr))
            prover.sync()
        except CityProverError:
            self.buf.free()
            flags.free()
            raise
        return self, flags

    @classmethod
    def view(cls, prover, ptr, n):
        self = cls.__new__(cls)
        self.prover, self.n, self.buf = prover, n, DeviceBuffer.view(prover, ptr, n * G2_AFFINE_BYTES // 8)
        return self

    def to_host(self, index=None):
        """the points (all, or those at `index`) as ((x0, x1), (y0, y1)) ints"""
        return [((c[0], c[1]), (c[2], c[3])) for c in _coords_to_host(self.buf, self.n, 4, index)]

    def msm_dev(self, scalars_ptr, inf_ptr=None):
        out, oi = np.zeros(24, np.uint64), ctypes.c_int()
        self.prover._check(self.prover.lib.cp_msm_bls12381_g2_dev(self.prover.ctx, scalars_ptr, self.buf.ptr, inf_ptr, self.n,
                                                                  _ptr(out), ctypes.byref(oi)))
        return _g2_out(out, oi)

    def free(self):
        self.buf.free()


# ---- NTT over the BLS12-381 scalar field ----
ABI["cp_ntt_bls12381_fr"] = (ctypes.c_int, [_vp, _u64p, ctypes.c_int, ctypes.c_uint, _u64p])
ABI["cp_ntt_bls12381_fr_dev"] = (ctypes.c_int, [_vp, _vp, ctypes.c_int, ctypes.c_uint, _u64p])
ABI["cp_groth16_quotient_bls12381_dev"] = (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_int])
ABI["cp_groth16_quotient_bls12381"] = (ctypes.c_int, [_vp, _u64p, _u64p, _u64p, ctypes.c_int])


def fr_ntt(prover, values, inverse=False, shift=None):
    """values: (n, 4) uint64 canonical F_r elements -> transformed copy (natural order). shift: coset shift (int)."""
    a = _as_u64(values).reshape(-1, 4).copy()
    log_n = int(a.shape[0]).bit_length() - 1
    flags = (NTT_INVERSE if inverse else 0) | (NTT_COSET if shift is not None else 0)
    sh = None if shift is None else np.array([(int(shift) >> (64 * j)) & (2**64 - 1) for j in range(4)], dtype=np.uint64)
    prover._check(prover.lib.cp_ntt_bls12381_fr(prover.ctx, _ptr(a), log_n, flags, None if sh is None else _ptr(sh)))
    return a


def fr_ntt_dev(prover, data_ptr, log_n, inverse=False, shift=None):
    flags = (NTT_INVERSE if inverse else 0) | (NTT_COSET if shift is not None else 0)
    sh = None if shift is None else np.array([(int(shift) >> (64 * j)) & (2**64 - 1) for j in range(4)], dtype=np.uint64)
    prover._check(prover.lib.cp_ntt_bls12381_fr_dev(prover.ctx, data_ptr, log_n, flags, None if sh is None else _ptr(sh)))


# ---- transforms of point vectors (the F_r NTT in the exponent) ----
ABI["cp_point_ntt_bls12381_g1_dev"] = (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, ctypes.c_uint])
ABI["cp_point_ntt_bls12381_g2_dev"] = (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, ctypes.c_uint])


def point_ntt_g1_dev(prover, points, flags_buf, log_n, inverse=False, flags=None):
    """cp_point_ntt_bls12381_g1_dev in place over a G1Points buffer of 2^log_n points and its flag buffer (as
    G1Points.fixed_base returns them). flags: the raw flag word instead of `inverse` (refusal tests). Asynchronous."""
    f = (NTT_INVERSE if inverse else 0) if flags is None else flags
    prover._check(prover.lib.cp_point_ntt_bls12381_g1_dev(prover.ctx, points.buf.ptr if points is not None else None,
                                                          flags_buf.ptr if flags_buf is not None else None, log_n, f))


def point_ntt_g2_dev(prover, points, flags_buf, log_n, inverse=False, flags=None):
    """point_ntt_g1_dev over a G2Points buffer (cp_point_ntt_bls12381_g2_dev)"""
    f = (NTT_INVERSE if inverse else 0) if flags is None else flags
    prover._check(prover.lib.cp_point_ntt_bls12381_g2_dev(prover.ctx, points.buf.ptr if points is not None else None,
                                                          flags_buf.ptr if flags_buf is not None else None, log_n, f))


def groth16_quotient(prover, a, b, c):
    """a, b, c: (n, 4) uint64 canonical F_r evaluations of (A w), (B w), (C w) on <omega_n> -> the n coefficients of
    h = (a b - c) / (x^n - 1) (cp_groth16_quotient_bls12381)."""
    a = _as_u64(a).reshape(-1, 4).copy()
    b = np.ascontiguousarray(_as_u64(b).reshape(-1, 4))
    c = np.ascontiguousarray(_as_u64(c).reshape(-1, 4))
    if not (a.shape == b.shape == c.shape):
        raise ValueError("a, b, c must have the same length")
    log_n = int(a.shape[0]).bit_length() - 1
    prover._check(prover.lib.cp_groth16_quotient_bls12381(prover.ctx, _ptr(a), _ptr(b), _ptr(c), log_n))
    return a


def groth16_quotient_dev(prover, a_ptr, b_ptr, c_ptr, log_n):
    prover._check(prover.lib.cp_groth16_quotient_bls12381_dev(prover.ctx, a_ptr, b_ptr, c_ptr, log_n))


class Groth16Pk(ctypes.Structure):
    _fields_ = [("n_wires", ctypes.c_size_t), ("n_private", ctypes.c_size_t), ("log_domain", ctypes.c_int),
                ("a_g1", _vp), ("b_g1", _vp), ("b_g2", _vp), ("k_g1", _vp), ("z_g1", _vp), ("a_inf", _vp), ("b_inf", _vp),
                ("alpha_g1", ctypes.c_uint64 * 12), ("beta_g1", ctypes.c_uint64 * 12), ("delta_g1", ctypes.c_uint64 * 12),
                ("beta_g2", ctypes.c_uint64 * 24), ("delta_g2", ctypes.c_uint64 * 24)]


ABI["cp_groth16_prove_bls12381"] = (ctypes.c_int, [_vp, ctypes.POINTER(Groth16Pk), _vp, _vp, _vp, _vp, _u64p, _u64p,
                                                   _u64p, _u64p, _u64p])


def groth16_prove(prover, pk, witness_ptr, a_ptr, b_ptr, c_ptr, r, s):
    """cp_groth16_prove_bls12381: pk = Groth16Pk; device pointers; r, s ints. Returns (A, B, C) as coordinate tuples of ints:
    A, C = (x, y); B = ((x0, x1), (y0, y1))."""
    lim = lambda v: np.array([(int(v) >> (64 * j)) & (2**64 - 1) for j in range(4)], dtype=np.uint64)
    oa, ob, oc = np.zeros(12, np.uint64), np.zeros(24, np.uint64), np.zeros(12, np.uint64)
    rr, ss = lim(r), lim(s)
    prover._check(prover.lib.cp_groth16_prove_bls12381(prover.ctx, ctypes.byref(pk), witness_ptr, a_ptr, b_ptr, c_ptr, _ptr(rr), _ptr(ss),
                                                       _ptr(oa), _ptr(ob), _ptr(oc)))
    val = lambda a: sum(int(v) << (64 * j) for j, v in enumerate(a))
    return ((val(oa[:6]), val(oa[6:])), ((val(ob[:6]), val(ob[6:12])), (val(ob[12:18]), val(ob[18:]))), (val(oc[:6]), val(oc[6:])))


# ---- the R1CS on the device: evaluations, satisfaction check, proof from a witness alone ----
_u32p = ctypes.POINTER(ctypes.c_uint32)
R1CS_NO_TERM_CLASSES = 1


class R1csMatrix(ctypes.Structure):
    _fields_ = [("row_ptr", _u64p), ("col", _u32p), ("coeff", _u32p)]


class R1csDesc(ctypes.Structure):
    _fields_ = [("n_constraints", ctypes.c_size_t), ("n_wires", ctypes.c_size_t), ("coeffs", _u64p), ("n_coeffs", ctypes.c_size_t),
                ("a", R1csMatrix), ("b", R1csMatrix), ("c", R1csMatrix), ("flags", ctypes.c_uint)]


class R1csInfo(ctypes.Structure):
    _fields_ = [("n_constraints", ctypes.c_size_t), ("n_wires", ctypes.c_size_t), ("n_coeffs", ctypes.c_size_t), ("log_domain", ctypes.c_int),
                ("nnz", ctypes.c_size_t * 3), ("longest_row", ctypes.c_size_t), ("device_bytes", ctypes.c_size_t),
                ("long_row_threshold", ctypes.c_size_t), ("n_short_rows", ctypes.c_size_t), ("n_long_rows", ctypes.c_size_t),
                ("n_terms_class", ctypes.c_size_t * 6)]


ABI["cp_r1cs_bls12381_create"] = (_vp, [_vp, ctypes.POINTER(R1csDesc)])
ABI["cp_r1cs_bls12381_destroy"] = (None, [_vp])
ABI["cp_r1cs_bls12381_get_info"] = (ctypes.c_int, [_vp, ctypes.POINTER(R1csInfo)])
ABI["cp_r1cs_bls12381_eval_dev"] = (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp])
ABI["cp_r1cs_bls12381_check_dev"] = (ctypes.c_int, [_vp, _vp, _vp, ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t)])
ABI["cp_groth16_prove_r1cs_bls12381"] = (ctypes.c_int, [_vp, ctypes.POINTER(Groth16Pk), _vp, _vp, _u64p, _u64p, _u64p, _u64p, _u64p])


def r1cs_desc(n_constraints, n_wires, coeffs, matrices, flags=0):
    """R1csDesc over numpy arrays. coeffs: (n_coeffs, 4) uint64; matrices: three (row_ptr uint64, col uint32, coeff uint32).
    Returns (desc, keep): `keep` holds the arrays the descriptor points into."""
    coeffs = np.ascontiguousarray(np.asarray(coeffs, dtype=np.uint64).reshape(-1, 4))
    d = R1csDesc()
    d.n_constraints, d.n_wires, d.n_coeffs, d.flags = int(n_constraints), int(n_wires), coeffs.shape[0], int(flags)
    d.coeffs = coeffs.ctypes.data_as(_u64p) if coeffs.size else None
    keep = [coeffs]
    for name, (row_ptr, col, coeff) in zip("abc", matrices):
        m = getattr(d, name)
        row_ptr = np.ascontiguousarray(np.asarray(row_ptr, dtype=np.uint64))
        col, coeff = (np.ascontiguousarray(np.asarray(x, dtype=np.uint32)) for x in (col, coeff))
        m.row_ptr = row_ptr.ctypes.data_as(_u64p)
        m.col = col.ctypes.data_as(_u32p) if col.size else None
        m.coeff = coeff.ctypes.data_as(_u32p) if coeff.size else None
        keep += [row_ptr, col, coeff]
    return d, keep


class R1cs:
    """A constraint system resident on the device (cp_r1cs_bls12381_create)."""

    def __init__(self, prover, n_constraints, n_wires, coeffs, matrices, flags=0):
        self.prover = prover
        desc, keep = r1cs_desc(n_constraints, n_wires, coeffs, matrices, flags)
        self.handle = prover.lib.cp_r1cs_bls12381_create(prover.ctx, ctypes.byref(desc))
        del keep
        if not self.handle:
            raise CityProverError(prover.lib.cp_last_error(None).decode())
        self.info = R1csInfo()
        prover._check(prover.lib.cp_r1cs_bls12381_get_info(self.handle, ctypes.byref(self.info)))
        self.n_pad = 1 << self.info.log_domain

    def eval_dev(self, witness_ptr, a_ptr, b_ptr, c_ptr):
        self.prover._check(self.prover.lib.cp_r1cs_bls12381_eval_dev(self.prover.ctx, self.handle, witness_ptr, a_ptr, b_ptr, c_ptr))

    def eval(self, witness_ptr):
        """A w, B w, C w as three (2^log_domain, 4) uint64 arrays"""
        bufs = [self.prover.alloc(4 * self.n_pad) for _ in range(3)]
        try:
            self.eval_dev(witness_ptr, *(b.ptr for b in bufs))
            return tuple(b.download().reshape(-1, 4) for b in bufs)
        finally:
            for b in bufs:
                b.free()

    def check(self, witness_ptr):
        """(number of violated constraints, the lowest violated one or None)"""
        n, first = ctypes.c_size_t(), ctypes.c_size_t()
        self.prover._check(self.prover.lib.cp_r1cs_bls12381_check_dev(self.prover.ctx, self.handle, witness_ptr, ctypes.byref(n), ctypes.byref(first)))
        return n.value, (first.value if n.value else None)

    def free(self):
        if self.handle:
            self.prover.lib.cp_r1cs_bls12381_destroy(self.handle)
            self.handle = None


def groth16_prove_r1cs(prover, pk, r1cs, witness_ptr, r, s, out=None):
    """cp_groth16_prove_r1cs_bls12381: the proof from (key, constraint system, witness). Returns (A, B, C) as groth16_prove does.
    out: optional (12, 24, 12)-word uint64 arrays to receive the raw coordinates (a refused call leaves them alone)."""
    lim = lambda v: np.array([(int(v) >> (64 * j)) & (2**64 - 1) for j in range(4)], dtype=np.uint64)
    oa, ob, oc = out if out is not None else (np.zeros(12, np.uint64), np.zeros(24, np.uint64), np.zeros(12, np.uint64))
    rr, ss = lim(r), lim(s)
    prover._check(prover.lib.cp_groth16_prove_r1cs_bls12381(prover.ctx, ctypes.byref(pk), r1cs.handle, witness_ptr, _ptr(rr), _ptr(ss),
                                                            _ptr(oa), _ptr(ob), _ptr(oc)))
    val = lambda a: sum(int(v) << (64 * j) for j, v in enumerate(a))
    return ((val(oa[:6]), val(oa[6:])), ((val(ob[:6]), val(ob[6:12])), (val(ob[12:18]), val(ob[18:]))), (val(oc[:6]), val(oc[6:])))


# ---- Groth16 setup: (constraint system, trapdoor) -> the proving key on the device and the verifying key ----
class Groth16Trapdoor(ctypes.Structure):
    _fields_ = [(name, ctypes.c_uint64 * 4) for name in ("tau", "alpha", "beta", "gamma", "delta")]


class Groth16Vk(ctypes.Structure):
    _fields_ = [("alpha_g1", ctypes.c_uint64 * 12), ("beta_g2", ctypes.c_uint64 * 24), ("gamma_g2", ctypes.c_uint64 * 24),
                ("delta_g2", ctypes.c_uint64 * 24), ("n_public", ctypes.c_size_t)]


ABI["cp_groth16_setup_bls12381"] = (_vp, [_vp, ctypes.POINTER(R1csDesc), ctypes.c_size_t, ctypes.POINTER(Groth16Trapdoor)])
ABI["cp_groth16_key_destroy"] = (None, [_vp])
ABI["cp_groth16_key_pk"] = (ctypes.c_int, [_vp, ctypes.POINTER(Groth16Pk)])
ABI["cp_groth16_key_vk"] = (ctypes.c_int, [_vp, ctypes.POINTER(Groth16Vk), _u64p, _u8p])


# ---- a key without a trapdoor: setup from a powers-of-tau SRS, delta contributions (include/cityprover.h) ----
GROTH16_SRS_CHECK_TORSION = 1


class Groth16SrsDesc(ctypes.Structure):
    _fields_ = [("log_size", ctypes.c_int), ("tau_g1", _u64p), ("tau_g2", _u64p), ("alpha_tau_g1", _u64p), ("beta_tau_g1", _u64p),
                ("beta_g2", ctypes.c_uint64 * 24)]


ABI["cp_groth16_srs_create_bls12381"] = (_vp, [_vp, ctypes.POINTER(Groth16SrsDesc), ctypes.c_uint])
ABI["cp_groth16_srs_destroy"] = (None, [_vp])
ABI["cp_groth16_setup_srs_bls12381"] = (_vp, [_vp, ctypes.POINTER(R1csDesc), ctypes.c_size_t, _vp])
ABI["cp_groth16_key_contribute_bls12381"] = (ctypes.c_int, [_vp, _vp, _u64p, ctypes.POINTER(_vp)])
ABI["cp_groth16_key_check_contribution_bls12381"] = (ctypes.c_int, [_vp, _vp, _vp, _u64p, ctypes.POINTER(ctypes.c_int)])
ABI["cp_groth16_srs_unit_bls12381"] = (_vp, [_vp, ctypes.c_int])
ABI["cp_groth16_srs_contribute_bls12381"] = (ctypes.c_int, [_vp, _vp, _u64p, _u64p, _u64p, ctypes.POINTER(_vp)])
ABI["cp_groth16_srs_points_bls12381"] = (ctypes.c_int, [_vp, _vp, ctypes.POINTER(ctypes.c_int), _u64p, _u64p, _u64p, _u64p, _u64p])
ABI["cp_groth16_srs_check_bls12381"] = (ctypes.c_int, [_vp, _vp, _u64p, ctypes.POINTER(ctypes.c_int)])


class Groth16Srs:
    """A phase-1 powers-of-tau SRS resident on the device (cp_groth16_srs_create_bls12381). Its points are checked one by one
    when it is created; check() tells whether the arrays belong together. unit() and contribute() make and extend one."""

    def __init__(self, prover, log_size, tau_g1, tau_g2, alpha_tau_g1, beta_tau_g1, beta_g2, check_torsion=False, flags=None):
        """tau_g1: (2^(L+1) - 1, 12) u64, tau_g2: (2^L, 24), alpha_tau_g1 / beta_tau_g1: (2^L, 12), beta_g2: 24 u64 - affine
        canonical. flags: the raw flag word instead of check_torsion (refusal tests)."""
        arrays = [_as_u64(a) for a in (tau_g1, tau_g2, alpha_tau_g1, beta_tau_g1)]
        n = 1 << log_size
        for a, want in zip(arrays, ((2 * n - 1) * 12, n * 24, n * 12, n * 12)):
            if a.size != want:
                raise ValueError("an SRS array has %d words, log_size %d needs %d" % (a.size, log_size, want))
        desc = Groth16SrsDesc()
        desc.log_size = log_size
        desc.tau_g1, desc.tau_g2, desc.alpha_tau_g1, desc.beta_tau_g1 = (_ptr(a) for a in arrays)
        desc.beta_g2[:] = [int(v) for v in _as_u64(beta_g2).reshape(24)]
        f = (GROTH16_SRS_CHECK_TORSION if check_torsion else 0) if flags is None else flags
        self.prover, self.log_size = prover, log_size
        self.handle = prover.lib.cp_groth16_srs_create_bls12381(prover.ctx, ctypes.byref(desc), f)
        del arrays
        if not self.handle:
            raise CityProverError(prover.lib.cp_last_error(None).decode())

    @classmethod
    def _of_handle(cls, prover, log_size, handle):
        self = cls.__new__(cls)
        self.prover, self.log_size, self.handle = prover, log_size, handle
        return self

    @classmethod
    def unit(cls, prover, log_size):
        """cp_groth16_srs_unit_bls12381: the SRS of tau = alpha = beta = 1, the start of a ceremony (worthless as an SRS)"""
        handle = prover.lib.cp_groth16_srs_unit_bls12381(prover.ctx, int(log_size))
        if not handle:
            raise CityProverError(prover.lib.cp_last_error(None).decode())
        return cls._of_handle(prover, int(log_size), handle)

    def contribute(self, t, a, b, prover=None):
        """cp_groth16_srs_contribute_bls12381: a new Groth16Srs with tau, alpha, beta multiplied by the ints t, a, b (the caller's
        secrets); applied to unit() it is the SRS of (t, a, b)"""
        p = prover or self.prover
        s = [np.array([(int(v) >> (64 * j)) & (2**64 - 1) for j in range(4)], dtype=np.uint64) for v in (t, a, b)]
        out = ctypes.c_void_p()
        p._check(p.lib.cp_groth16_srs_contribute_bls12381(p.ctx, self.handle, _ptr(s[0]), _ptr(s[1]), _ptr(s[2]), ctypes.byref(out)))
        return Groth16Srs._of_handle(p, self.log_size, out.value)

    def points(self, prover=None):
        """cp_groth16_srs_points_bls12381: the five parts of cp_groth16_srs_desc as a dict of u64 arrays, affine canonical - what
        __init__ takes"""
        p = prover or self.prover
        L = ctypes.c_int(-1)
        p._check(p.lib.cp_groth16_srs_points_bls12381(p.ctx, self.handle, ctypes.byref(L), None, None, None, None, None))
        n = 1 << L.value
        out = {"log_size": L.value, "tau_g1": np.zeros((2 * n - 1, 12), np.uint64), "tau_g2": np.zeros((n, 24), np.uint64),
               "alpha_tau_g1": np.zeros((n, 12), np.uint64), "beta_tau_g1": np.zeros((n, 12), np.uint64), "beta_g2": np.zeros(24, np.uint64)}
        p._check(p.lib.cp_groth16_srs_points_bls12381(p.ctx, self.handle, None, _ptr(out["tau_g1"]), _ptr(out["tau_g2"]), _ptr(out["alpha_tau_g1"]),
                                                      _ptr(out["beta_tau_g1"]), _ptr(out["beta_g2"])))
        return out

    def check(self, weights, prover=None):
        """cp_groth16_srs_check_bls12381: (verdict, reason). weights: 5 * 2^log_size - 5 non-zero ints below 2^128 (or an (n, 2) u64
        array), one per adjacent pair of tau_g1, tau_g2, alpha_tau_g1, beta_tau_g1 in this order, unpredictable to whoever made
        the SRS."""
        p = prover or self.prover
        w = None
        if weights is not None:
            w = _as_u64(weights).reshape(-1, 2) if isinstance(weights, np.ndarray) else _weights128(weights, len(weights))
            if w.shape[0] != 5 * (1 << self.log_size) - 5:
                raise ValueError("an SRS of log_size %d takes %d weights, not %d" % (self.log_size, 5 * (1 << self.log_size) - 5, w.shape[0]))
        verdict = ctypes.c_int(-1)
        p._check(p.lib.cp_groth16_srs_check_bls12381(p.ctx, self.handle, None if w is None else _ptr(w), ctypes.byref(verdict)))
        return verdict.value, p.lib.cp_last_error(p.ctx).decode()

    def free(self):
        if self.handle:
            self.prover.lib.cp_groth16_srs_destroy(self.handle)
            self.handle = None


class Groth16Key:
    """A proving key resident on the device, with its verifying key (cp_groth16_setup_bls12381)."""

    def __init__(self, prover, handle):
        self.prover, self.handle = prover, handle

    @classmethod
    def setup(cls, prover, n_constraints, n_wires, coeffs, matrices, n_public, tau, alpha, beta, gamma, delta, flags=0):
        """The system as R1cs takes it; n_public counts wire 0; the five trapdoor scalars are ints (the caller's randomness)."""
        desc, keep = r1cs_desc(n_constraints, n_wires, coeffs, matrices, flags)
        td = Groth16Trapdoor()
        for name, v in (("tau", tau), ("alpha", alpha), ("beta", beta), ("gamma", gamma), ("delta", delta)):
            getattr(td, name)[:] = [(int(v) >> (64 * j)) & (2**64 - 1) for j in range(4)]
        handle = prover.lib.cp_groth16_setup_bls12381(prover.ctx, ctypes.byref(desc), int(n_public), ctypes.byref(td))
        del keep
        if not handle:
            raise CityProverError(prover.lib.cp_last_error(None).decode())
        return cls(prover, handle)

    @classmethod
    def setup_srs(cls, prover, n_constraints, n_wires, coeffs, matrices, n_public, srs, flags=0):
        """cp_groth16_setup_srs_bls12381: the key of (tau, alpha, beta, gamma = 1, delta = 1) from a Groth16Srs, without any secret"""
        desc, keep = r1cs_desc(n_constraints, n_wires, coeffs, matrices, flags)
        handle = prover.lib.cp_groth16_setup_srs_bls12381(prover.ctx, ctypes.byref(desc), int(n_public), srs.handle)
        del keep
        if not handle:
            raise CityProverError(prover.lib.cp_last_error(None).decode())
        return cls(prover, handle)

    def contribute(self, d, prover=None):
        """cp_groth16_key_contribute_bls12381: a new key with delta multiplied by the int d (the caller's secret), K and Z by 1 / d"""
        p = prover or self.prover
        dd = np.array([(int(d) >> (64 * j)) & (2**64 - 1) for j in range(4)], dtype=np.uint64)
        out = ctypes.c_void_p()
        p._check(p.lib.cp_groth16_key_contribute_bls12381(p.ctx, self.handle, _ptr(dd), ctypes.byref(out)))
        return Groth16Key(p, out.value)

    @staticmethod
    def check_contribution(prover, before, after, weights):
        """cp_groth16_key_check_contribution_bls12381: (verdict, reason). weights: n_private + 2^log_domain - 1 non-zero ints below
        2^128 (or an (n, 2) u64 array), unpredictable to whoever made `after`."""
        w = None
        if weights is not None:
            w = _as_u64(weights).reshape(-1, 2) if isinstance(weights, np.ndarray) else _weights128(weights, len(weights))
        verdict = ctypes.c_int(-1)
        prover._check(prover.lib.cp_groth16_key_check_contribution_bls12381(prover.ctx, before.handle, after.handle,
                                                                            None if w is None else _ptr(w), ctypes.byref(verdict)))
        return verdict.value, prover.lib.cp_last_error(prover.ctx).decode()

    def pk(self):
        """Groth16Pk: a view, valid until free()"""
        pk = Groth16Pk()
        self.prover._check(self.prover.lib.cp_groth16_key_pk(self.handle, ctypes.byref(pk)))
        return pk

    def vk(self):
        """dict: alpha_g1, beta_g2, gamma_g2, delta_g2 as coordinate tuples of ints, n_public, ic: n_public points (None = infinity)"""
        vk = Groth16Vk()
        self.prover._check(self.prover.lib.cp_groth16_key_vk(self.handle, ctypes.byref(vk), None, None))
        n = vk.n_public
        xy, inf = np.zeros((n, 12), np.uint64), np.zeros(n, np.uint8)
        self.prover._check(self.prover.lib.cp_groth16_key_vk(self.handle, ctypes.byref(vk), _ptr(xy), inf.ctypes.data_as(_u8p)))
        val = lambda a: sum(int(v) << (64 * j) for j, v in enumerate(a))
        g2 = lambda a: ((val(a[0:6]), val(a[6:12])), (val(a[12:18]), val(a[18:24])))
        return {"alpha_g1": (val(vk.alpha_g1[0:6]), val(vk.alpha_g1[6:12])), "beta_g2": g2(vk.beta_g2), "gamma_g2": g2(vk.gamma_g2),
                "delta_g2": g2(vk.delta_g2), "n_public": n,
                "ic": [None if inf[i] else (val(xy[i, :6]), val(xy[i, 6:])) for i in range(n)]}

    def point_sets(self):
        """the five sets as G1Points / G2Points views and the two flag arrays as uint8 (tests, inspection)"""
        pk, p = self.pk(), self.prover
        n_z = (1 << pk.log_domain) - 1
        return {"a_g1": G1Points.view(p, pk.a_g1, pk.n_wires), "b_g1": G1Points.view(p, pk.b_g1, pk.n_wires),
                "b_g2": G2Points.view(p, pk.b_g2, pk.n_wires), "k_g1": G1Points.view(p, pk.k_g1, pk.n_private),
                "z_g1": G1Points.view(p, pk.z_g1, n_z),
                "a_inf": flags_to_host(DeviceBuffer.view(p, pk.a_inf, (pk.n_wires + 7) // 8), pk.n_wires),
                "b_inf": flags_to_host(DeviceBuffer.view(p, pk.b_inf, (pk.n_wires + 7) // 8), pk.n_wires)}

    def save(self, path, raw=False, chunk_points=0):
        """cp_groth16_key_save_file: the key as a file (include/cityprover.h has the layout), compressed points unless raw;
        chunk_points: points per device pass (0: the library's default)"""
        flags = GROTH16_KEY_FILE_RAW if raw else 0
        self.prover._check(self.prover.lib.cp_groth16_key_save_file(self.prover.ctx, self.handle, os.fsencode(path), flags, int(chunk_points)))

    @classmethod
    def load(cls, prover, path, check_torsion=False, chunk_points=0):
        """cp_groth16_key_load_file: a key like the one setup() returns, from a file and without the trapdoor; check_torsion
        also holds every point of the five sets to [r]P = infinity"""
        flags = GROTH16_KEY_LOAD_CHECK_TORSION if check_torsion else 0
        handle = prover.lib.cp_groth16_key_load_file(prover.ctx, os.fsencode(path), flags, int(chunk_points))
        if not handle:
            raise CityProverError(prover.lib.cp_last_error(None).decode())
        return cls(prover, handle)

    def free(self):
        if self.handle:
            self.prover.lib.cp_groth16_key_destroy(self.handle)
            self.handle = None


# ---- Groth16 keys as files ----
GROTH16_KEY_FILE_VERSION = 1
GROTH16_KEY_FILE_RAW = 1
GROTH16_KEY_LOAD_CHECK_TORSION = 1


class Groth16KeyFileInfo(ctypes.Structure):
    _fields_ = [("version", ctypes.c_uint32), ("flags", ctypes.c_uint), ("log_domain", ctypes.c_int), ("n_wires", ctypes.c_size_t),
                ("n_public", ctypes.c_size_t), ("n_private", ctypes.c_size_t), ("file_bytes", ctypes.c_size_t), ("checksum", ctypes.c_uint64)]


ABI["cp_groth16_key_save_file"] = (ctypes.c_int, [_vp, _vp, ctypes.c_char_p, ctypes.c_uint, ctypes.c_size_t])
ABI["cp_groth16_key_load_file"] = (_vp, [_vp, ctypes.c_char_p, ctypes.c_uint, ctypes.c_size_t])
ABI["cp_groth16_key_file_info"] = (ctypes.c_int, [ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(Groth16KeyFileInfo), ctypes.POINTER(Groth16Vk), _u64p, _u8p])


def groth16_key_file_info(path, verify_checksum=True):
    """cp_groth16_key_file_info: parse and validate a key file on the host (no GPU, no square roots). Returns a dict: the header's
    fields, "vk" (Groth16Vk), "ic_xy" ((n_public, 12) u64) and "ic_inf" (n_public flags): what Groth16Verifier.create takes.
    Raises on a bad file."""
    lib = load_library()
    info, vk = Groth16KeyFileInfo(), Groth16Vk()
    rc = lib.cp_groth16_key_file_info(os.fsencode(path), int(bool(verify_checksum)), ctypes.byref(info), ctypes.byref(vk), None, None)
    if rc != 0:
        raise CityProverError(f"[{rc}] " + lib.cp_last_error(None).decode())
    xy, inf = np.zeros((vk.n_public, 12), np.uint64), np.zeros(vk.n_public, np.uint8)
    rc = lib.cp_groth16_key_file_info(os.fsencode(path), 0, None, None, _ptr(xy), inf.ctypes.data_as(_u8p))
    if rc != 0:
        raise CityProverError(f"[{rc}] " + lib.cp_last_error(None).decode())
    out = {name: getattr(info, name) for name, _ in Groth16KeyFileInfo._fields_}
    out.update(vk=vk, ic_xy=xy, ic_inf=inf)
    return out


# ---- pairing products and the Groth16 verifier (GT values are e(P, Q)^3: include/cityprover.h) ----
GT_WORDS = 72
PAIRING_TRUSTED = 1
ABI["cp_pairing_product_bls12381"] = (ctypes.c_int, [_vp, _u64p, _u8p, _u64p, _u8p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint, _u64p, _u8p, _u8p])
ABI["cp_groth16_verifier_create_bls12381"] = (_vp, [_vp, ctypes.POINTER(Groth16Vk), _u64p, _u8p])
ABI["cp_groth16_verifier_destroy"] = (None, [_vp])
ABI["cp_groth16_verify_bls12381"] = (ctypes.c_int, [_vp, _vp, _u64p, _u64p, ctypes.c_size_t, ctypes.c_uint, _u8p])


def _u8_or_none(a):
    return None if a is None else a.ctypes.data_as(_u8p)


def pairing_product(prover, g1_xy, g2_xy, k=1, g1_inf=None, g2_inf=None, flags=0, want_gt=True):
    """cp_pairing_product_bls12381. g1_xy: (n_products * k, 12) u64, g2_xy: (n_products * k, 24) u64, affine canonical; the
    optional flags are uint8 arrays of n_products * k. Returns (gt, is_one, status): gt is (n_products, 72) u64 or None."""
    g1_xy, g2_xy = _as_u64(g1_xy).reshape(-1, 12), _as_u64(g2_xy).reshape(-1, 24)
    assert len(g1_xy) == len(g2_xy) and k >= 1 and len(g1_xy) % k == 0
    n = len(g1_xy) // k
    f1 = None if g1_inf is None else np.ascontiguousarray(g1_inf, np.uint8)
    f2 = None if g2_inf is None else np.ascontiguousarray(g2_inf, np.uint8)
    gt = np.zeros((n, GT_WORDS), np.uint64) if want_gt else None
    is_one, status = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    prover._check(prover.lib.cp_pairing_product_bls12381(prover.ctx, _ptr(g1_xy), _u8_or_none(f1), _ptr(g2_xy), _u8_or_none(f2), n, k, flags,
                                                         None if gt is None else _ptr(gt), _u8_or_none(is_one), _u8_or_none(status)))
    return gt, is_one, status


class Groth16Verifier:
    """The verifier of one verifying key, resident on the device (cp_groth16_verifier_create_bls12381)."""

    def __init__(self, prover, handle, n_public):
        self.prover, self.handle, self.n_public = prover, handle, n_public

    @classmethod
    def create(cls, prover, vk, ic_xy, ic_inf=None):
        """vk: Groth16Vk; ic_xy: (n_public, 12) u64; ic_inf: n_public flags or None"""
        ic_xy = _as_u64(ic_xy).reshape(-1, 12)
        inf = None if ic_inf is None else np.ascontiguousarray(ic_inf, np.uint8)
        handle = prover.lib.cp_groth16_verifier_create_bls12381(prover.ctx, ctypes.byref(vk), _ptr(ic_xy), _u8_or_none(inf))
        if not handle:
            raise CityProverError(prover.lib.cp_last_error(None).decode())
        return cls(prover, handle, int(vk.n_public))

    @classmethod
    def from_key(cls, prover, key):
        """from a Groth16Key (cp_groth16_key_vk)"""
        vk = Groth16Vk()
        prover._check(prover.lib.cp_groth16_key_vk(key.handle, ctypes.byref(vk), None, None))
        xy, inf = np.zeros((vk.n_public, 12), np.uint64), np.zeros(vk.n_public, np.uint8)
        prover._check(prover.lib.cp_groth16_key_vk(key.handle, ctypes.byref(vk), _ptr(xy), inf.ctypes.data_as(_u8p)))
        return cls.create(prover, vk, xy, inf)

    def verify(self, proofs, publics=None, flags=0, prover=None):
        """proofs: (n, 48) u64, A | B | C; publics: (n, n_public - 1, 4) u64 (None when the key has no public input beside wire 0).
        Returns the n verdicts as uint8: 0 accepted, 1 rejected, 2 bad point, 3 outside the subgroup, 4 public input >= r.
        prover: another context of the same device (default: the one the verifier was made with)."""
        p = prover or self.prover
        proofs = _as_u64(proofs).reshape(-1, 48)
        n = len(proofs)
        pub = None
        if self.n_public > 1:
            pub = _as_u64(publics).reshape(n, self.n_public - 1, 4)
        out = np.zeros(n, np.uint8)
        p._check(p.lib.cp_groth16_verify_bls12381(p.ctx, self.handle, _ptr(proofs), None if pub is None else _ptr(pub), n, flags, out.ctypes.data_as(_u8p)))
        return out

    def verify_city(self, blobs, publics=None, flags=0, prover=None):
        """verify() with the proofs as stored: a sequence of 192-byte strings or an (n, 192) uint8 array
        (cp_groth16_verify_city_bls12381). A proof that does not decompress gets verdict 2."""
        p = prover or self.prover
        blobs = _city_blobs(blobs)
        n = len(blobs)
        pub = None
        if self.n_public > 1:
            pub = _as_u64(publics).reshape(n, self.n_public - 1, 4)
        out = np.zeros(n, np.uint8)
        p._check(p.lib.cp_groth16_verify_city_bls12381(p.ctx, self.handle, blobs.ctypes.data_as(_u8p), None if pub is None else _ptr(pub), n, flags,
                                                       out.ctypes.data_as(_u8p)))
        return out

    def _verify_all(self, fn, proofs, n, weights, publics, flags, prover):
        p = prover or self.prover
        pub = None
        if self.n_public > 1:
            pub = _as_u64(publics).reshape(n, self.n_public - 1, 4)
        w = _weights128(weights, n)
        out, path = np.zeros(n, np.uint8), ctypes.c_int(-1)
        p._check(getattr(p.lib, fn)(p.ctx, self.handle, proofs, None if pub is None else _ptr(pub), n, _ptr(w), flags, out.ctypes.data_as(_u8p),
                                    ctypes.byref(path)))
        return out, path.value

    def verify_all(self, proofs, weights, publics=None, flags=0, prover=None):
        """verify() under one final exponentiation (cp_groth16_verify_all_bls12381). weights: one non-zero 128-bit value per proof,
        as n ints or an (n, 2) u64 array; they must be unpredictable to whoever made the proofs (e.g. secrets.randbits(128)).
        Returns (verdicts, path): path 0 when the aggregated equation held, 1 when the per-proof check had to decide."""
        proofs = _as_u64(proofs).reshape(-1, 48)
        return self._verify_all("cp_groth16_verify_all_bls12381", _ptr(proofs), len(proofs), weights, publics, flags, prover)

    def verify_all_city(self, blobs, weights, publics=None, flags=0, prover=None):
        """verify_all() with the proofs as stored (cp_groth16_verify_all_city_bls12381)"""
        blobs = _city_blobs(blobs)
        return self._verify_all("cp_groth16_verify_all_city_bls12381", blobs.ctypes.data_as(_u8p), len(blobs), weights, publics, flags, prover)

    def close(self):
        if self.handle:
            self.prover.lib.cp_groth16_verifier_destroy(self.handle)
            self.handle = None


ABI["cp_groth16_proofs_unpack_city_bls12381"] = (ctypes.c_int, [_vp, _u8p, ctypes.c_size_t, _u64p, _u8p])
ABI["cp_groth16_verify_city_bls12381"] = (ctypes.c_int, [_vp, _vp, _u8p, _u64p, ctypes.c_size_t, ctypes.c_uint, _u8p])
ABI["cp_groth16_verify_all_bls12381"] = (ctypes.c_int, [_vp, _vp, _u64p, _u64p, ctypes.c_size_t, _u64p, ctypes.c_uint, _u8p, ctypes.POINTER(ctypes.c_int)])
ABI["cp_groth16_verify_all_city_bls12381"] = (ctypes.c_int, [_vp, _vp, _u8p, _u64p, ctypes.c_size_t, _u64p, ctypes.c_uint, _u8p, ctypes.POINTER(ctypes.c_int)])


def _weights128(weights, n):
    """n ints below 2^128 or an (n, 2) u64 array -> a contiguous (n, 2) u64 array"""
    if isinstance(weights, np.ndarray):
        return _as_u64(weights).reshape(n, 2)
    weights = [int(w) for w in weights]
    if len(weights) != n or any(w < 0 or w >> 128 for w in weights):
        raise ValueError("one weight of at most 128 bits per proof")
    return np.array([[w & (2**64 - 1), w >> 64] for w in weights], np.uint64).reshape(n, 2)


def _city_blobs(blobs):
    """a sequence of 192-byte strings or an (n, 192) uint8 array -> a contiguous (n, 192) uint8 array"""
    if isinstance(blobs, np.ndarray):
        a = np.ascontiguousarray(blobs, np.uint8)
    else:
        blobs = [bytes(b) for b in blobs]
        if any(len(b) != 192 for b in blobs):
            raise ValueError("CityGroth16ProofData is 192 bytes")
        a = np.frombuffer(b"".join(blobs), dtype=np.uint8).copy()
    if a.size % 192 or (a.ndim == 2 and a.shape[1] != 192) or a.ndim > 2:
        raise ValueError("CityGroth16ProofData is 192 bytes")
    return a.reshape(-1, 192)


def groth16_unpack_city_batch(prover, blobs):
    """cp_groth16_proofs_unpack_city_bls12381: stored proofs (a sequence of 192-byte strings or an (n, 192) uint8 array),
    decompressed on the device. Returns (coords (n, 48) u64: A | B | C as Groth16Verifier.verify takes them, status (n,) u8:
    0 ok, 1 a flag bit that may not be set, 2 an x >= p, 3 an x of no point); a proof whose status is not 0 has zero words."""
    blobs = _city_blobs(blobs)
    n = len(blobs)
    coords, status = np.zeros((n, 48), np.uint64), np.zeros(n, np.uint8)
    prover._check(prover.lib.cp_groth16_proofs_unpack_city_bls12381(prover.ctx, blobs.ctypes.data_as(_u8p), n, _ptr(coords), status.ctypes.data_as(_u8p)))
    return coords, status


# ---- circuit files (N1) and the stored Groth16 proof form ----
ABI["cp_circuit_load_file"] = (_vp, [_vp, ctypes.c_char_p])
ABI["cp_circuit_save_file"] = (ctypes.c_int, [_vp, ctypes.c_char_p])
ABI["cp_circuit_file_info"] = (ctypes.c_int, [ctypes.c_char_p, ctypes.POINTER(Shape), _u64p, ctypes.POINTER(ctypes.c_size_t),
                                              ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_uint)])
ABI["cp_circuit_set_public_input_targets"] = (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_uint32), ctypes.c_size_t])
ABI["cp_circuit_public_inputs_from_wires"] = (ctypes.c_int, [_vp, _u64p, _u64p])
ABI["cp_circuit_shape"] = (ctypes.c_int, [_vp, ctypes.POINTER(Shape), _u64p])
ABI["cp_groth16_proof_pack_city"] = (ctypes.c_int, [_u64p, _u64p, _u64p, _u8p])
ABI["cp_groth16_proof_unpack_city"] = (ctypes.c_int, [_u8p, _u64p, _u64p, _u64p])


def circuit_file_info(path):
    """cp_circuit_file_info: parse + validate a .cpcirc file on the host (no GPU). Returns a dict; raises on a bad file."""
    lib = load_library()
    sh, dg = Shape(), np.zeros(4, np.uint64)
    ng, ns, fl = ctypes.c_size_t(), ctypes.c_int(), ctypes.c_uint()
    rc = lib.cp_circuit_file_info(os.fsencode(path), ctypes.byref(sh), _ptr(dg), ctypes.byref(ng), ctypes.byref(ns), ctypes.byref(fl))
    if rc != 0:
        raise CityProverError(f"[{rc}] " + lib.cp_last_error(None).decode())
    return dict(shape=sh, digest=[int(x) for x in dg], n_gates=ng.value, num_selectors=ns.value, flags=fl.value)


def load_circuit_file(prover, path):
    """cp_circuit_load_file -> Circuit"""
    h = prover.lib.cp_circuit_load_file(prover.ctx, os.fsencode(path))
    if not h:
        raise CityProverError(prover.lib.cp_last_error(prover.ctx).decode())
    c = Circuit.__new__(Circuit)
    c.prover, c.handle, c.shape = prover, h, Shape()
    prover._check(prover.lib.cp_circuit_shape(h, ctypes.byref(c.shape), None))
    c.n_gates = circuit_file_info(path)["n_gates"]
    return c


def save_circuit_file(circuit, path):
    circuit.prover._check(circuit.prover.lib.cp_circuit_save_file(circuit.handle, os.fsencode(path)))


def set_public_input_targets(circuit, row_wire_pairs):
    t = np.ascontiguousarray(np.asarray(row_wire_pairs, dtype=np.uint32).reshape(-1, 2))
    circuit.prover._check(circuit.prover.lib.cp_circuit_set_public_input_targets(
        circuit.handle, t.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), t.shape[0]))


def public_inputs_from_wires(circuit, wires):
    w = _as_u64(wires)
    out = np.zeros(circuit.shape.num_public_inputs, np.uint64)
    circuit.prover._check(circuit.prover.lib.cp_circuit_public_inputs_from_wires(circuit.handle, _ptr(w), _ptr(out) if out.size else None))
    return out


def _limbs6(v):
    return [(int(v) >> (64 * i)) & (2**64 - 1) for i in range(6)]


def groth16_pack_city(A, B, C):
    """(A, B, C) as groth16_prove returns them -> the 192 bytes of CityGroth16ProofData (pi_a | pi_b_a0 | pi_b_a1 | pi_c)."""
    lib = load_library()
    a = np.array(_limbs6(A[0]) + _limbs6(A[1]), dtype=np.uint64)
    b = np.array(_limbs6(B[0][0]) + _limbs6(B[0][1]) + _limbs6(B[1][0]) + _limbs6(B[1][1]), dtype=np.uint64)
    c = np.array(_limbs6(C[0]) + _limbs6(C[1]), dtype=np.uint64)
    out = np.zeros(192, np.uint8)
    rc = lib.cp_groth16_proof_pack_city(_ptr(a), _ptr(b), _ptr(c), out.ctypes.data_as(_u8p))
    if rc != 0:
        raise CityProverError(f"[{rc}] " + lib.cp_last_error(None).decode())
    return out.tobytes()


def groth16_unpack_city(data):
    lib = load_library()
    buf = np.frombuffer(bytes(data), dtype=np.uint8).copy()
    if buf.size != 192:
        raise ValueError("CityGroth16ProofData is 192 bytes")
    a, b, c = np.zeros(12, np.uint64), np.zeros(24, np.uint64), np.zeros(12, np.uint64)
    rc = lib.cp_groth16_proof_unpack_city(buf.ctypes.data_as(_u8p), _ptr(a), _ptr(b), _ptr(c))
    if rc != 0:
        raise CityProverError(f"[{rc}] " + lib.cp_last_error(None).decode())
    val = lambda x: sum(int(v) << (64 * j) for j, v in enumerate(x))
    return ((val(a[:6]), val(a[6:])), ((val(b[:6]), val(b[6:12])), (val(b[12:18]), val(b[18:]))), (val(c[:6]), val(c[6:])))


# ---- FRI primitives and the verifier's audit hook ----
ABI["cp_verify_fri_queries_with_challenges"] = (ctypes.c_int, [ctypes.POINTER(Shape), ctypes.c_char_p, ctypes.c_size_t, _u64p, _u64p, _u64p, _u64p])
ABI["cp_fri_combine_dev"] = (ctypes.c_int, [_vp, _vp, ctypes.c_size_t, ctypes.c_size_t, _u64p, _vp])
ABI["cp_fri_fold_dev"] = (ctypes.c_int, [_vp, _vp, ctypes.c_size_t, ctypes.c_int, _u64p, _vp])


def verify_fri_queries_with_challenges(shape, proof_bytes, alpha, zeta, fri_betas, x_indices):
    """cp_verify's query phase with supplied challenges (no circuit, no GPU). Raises CityProverError on rejection."""
    lib = load_library()
    a, z = _as_u64(alpha), _as_u64(zeta)
    fb = _as_u64(fri_betas).reshape(-1)
    xi = _as_u64(x_indices)
    rc = lib.cp_verify_fri_queries_with_challenges(ctypes.byref(shape), proof_bytes, len(proof_bytes), _ptr(a), _ptr(z),
                                                   _ptr(fb) if fb.size else None, _ptr(xi))
    if rc != 0:
        raise CityProverError(f"[{rc}] " + lib.cp_last_error(None).decode())


# ---- batches of proofs of one circuit: the query phase on the device (cp_verify_batch) ----
_u8pp = ctypes.POINTER(ctypes.c_char_p)
_szp = ctypes.POINTER(ctypes.c_size_t)
ABI["cp_verify_batch"] = (ctypes.c_int, [_vp, _u8pp, _szp, ctypes.c_size_t, ctypes.c_size_t, _vp])
ABI["cp_verify_fri_queries_with_challenges_batch"] = (ctypes.c_int, [_vp, ctypes.POINTER(Shape), _u64p, _u8pp, _szp, ctypes.c_size_t, _u64p, _u64p,
                                                                     _u64p, _u64p, ctypes.c_size_t, _vp])
# cp_verify_verdict; status: 0 accepted, 1 malformed, 2 element >= p, 3 public inputs, 4 zeta in the subgroup / opening point on the
# coset, 5 vanishing identity, 6 proof of work, 7 oracle path, 8 FRI layer value, 9 FRI layer path, 10 final polynomial
VERDICT = np.dtype([("status", np.int32), ("query", np.int32), ("detail", np.int32), ("reserved", np.int32)])


def _proof_array(proofs):
    proofs = [bytes(b) for b in proofs]
    ptrs = (ctypes.c_char_p * max(len(proofs), 1))(*proofs)
    lens = (ctypes.c_size_t * max(len(proofs), 1))(*[len(b) for b in proofs])
    return proofs, ptrs, lens


def verify_batch(circuit, proofs, chunk=0):
    """cp_verify_batch: one verdict per proof (structured array, dtype VERDICT); raises only for a call that could not run."""
    keep, ptrs, lens = _proof_array(proofs)
    out = np.zeros(len(keep), VERDICT)
    p = circuit.prover
    p._check(p.lib.cp_verify_batch(circuit.handle, ptrs, lens, len(keep), int(chunk), out.ctypes.data))
    return out


def verify_fri_queries_with_challenges_batch(prover, shape, proofs, alphas, zetas, fri_betas, x_indices, cs_cap=None, chunk=0):
    """cp_verify_fri_queries_with_challenges_batch: the device twin of verify_fri_queries_with_challenges for n proofs of one
    shape. alphas, zetas: (n, 2); fri_betas: (n, n_arity, 2); x_indices: (n, num_query_rounds). Returns the verdicts."""
    keep, ptrs, lens = _proof_array(proofs)
    n = len(keep)
    a, z, fb, xi = _as_u64(alphas).reshape(-1), _as_u64(zetas).reshape(-1), _as_u64(fri_betas).reshape(-1), _as_u64(x_indices).reshape(-1)
    cap = None if cs_cap is None else _as_u64(cs_cap).reshape(-1)
    out = np.zeros(n, VERDICT)
    prover._check(prover.lib.cp_verify_fri_queries_with_challenges_batch(
        prover.ctx, ctypes.byref(shape), None if cap is None else _ptr(cap), ptrs, lens, n, _ptr(a) if a.size else None, _ptr(z) if z.size else None,
        _ptr(fb) if fb.size else None, _ptr(xi) if xi.size else None, int(chunk), out.ctypes.data))
    return out


def fri_combine(prover, polys, alpha):
    """sum_j alpha^j polys[j] over F_p^2 on the GPU (cp_fri_combine_dev). polys: (k, n) uint64 -> (n, 2) uint64."""
    f = _as_u64(polys)
    k, n = f.shape
    din, dout = prover.to_device(f), prover.alloc(2 * n)
    try:
        a = _as_u64(alpha)
        prover._check(prover.lib.cp_fri_combine_dev(prover.ctx, din.ptr, k, n, _ptr(a), dout.ptr))
        return dout.download().reshape(n, 2)
    finally:
        din.free()
        dout.free()


def fri_fold(prover, coeffs_re_im, arity_bits, beta):
    """one FRI reduction layer in coefficient space (cp_fri_fold_dev). coeffs_re_im: (2, n_in) uint64 -> (2, n_in >> arity_bits)."""
    c = _as_u64(coeffs_re_im)
    n_in = c.shape[1]
    din, dout = prover.to_device(c), prover.alloc(2 * (n_in >> arity_bits))
    try:
        b = _as_u64(beta)
        prover._check(prover.lib.cp_fri_fold_dev(prover.ctx, din.ptr, n_in, arity_bits, _ptr(b), dout.ptr))
        return dout.download().reshape(2, n_in >> arity_bits)
    finally:
        din.free()
        dout.free()


# ---- the two plonky2-level seams: PolynomialBatch handles and prove_openings / verify_fri_proof -------------------
class ChallengerState(ctypes.Structure):
    """cp_challenger_state: plonky2 `Challenger` by value (sponge state, pending inputs, unread outputs)."""
    _fields_ = [("sponge_state", ctypes.c_uint64 * 12), ("input_buffer", ctypes.c_uint64 * 8),
                ("output_buffer", ctypes.c_uint64 * 8), ("n_input", ctypes.c_uint32), ("n_output", ctypes.c_uint32)]

    def observe(self, elements):
        e = _as_u64(elements).ravel()
        lib = load_library()
        rc = lib.cp_challenger_observe(ctypes.byref(self), _ptr(e) if e.size else None, e.size)
        if rc != 0:
            raise CityProverError(f"[{rc}] " + lib.cp_last_error(None).decode())
        return self

    def challenges(self, count):
        out = np.zeros(count, np.uint64)
        lib = load_library()
        rc = lib.cp_challenger_challenges(ctypes.byref(self), _ptr(out), count)
        if rc != 0:
            raise CityProverError(f"[{rc}] " + lib.cp_last_error(None).decode())
        return out

    def ext_challenge(self):
        return self.challenges(2)

    def copy(self):
        c = ChallengerState()
        ctypes.memmove(ctypes.byref(c), ctypes.byref(self), ctypes.sizeof(ChallengerState))
        return c

    def as_tuple(self):
        return (tuple(self.sponge_state), tuple(self.input_buffer[:self.n_input]), tuple(self.output_buffer[:self.n_output]))


class FriParams(ctypes.Structure):
    """cp_fri_params (plonky2 FriParams)."""
    _fields_ = [(n, ctypes.c_int) for n in ("degree_bits", "rate_bits", "cap_height", "pow_bits", "num_query_rounds", "n_arity")] + [
        ("arity_bits", ctypes.c_int * 8)]


def fri_params(degree_bits, rate_bits, cap_height, pow_bits, num_query_rounds, arity_bits):
    p = FriParams(degree_bits, rate_bits, cap_height, pow_bits, num_query_rounds, len(arity_bits))
    for i, a in enumerate(arity_bits):
        p.arity_bits[i] = a
    return p


class FriPolyRange(ctypes.Structure):
    _fields_ = [("oracle", ctypes.c_uint32), ("first", ctypes.c_uint32), ("count", ctypes.c_uint32)]


class FriBatch(ctypes.Structure):
    """cp_fri_batch (plonky2 FriBatchInfo with the polynomial list as runs)."""
    _fields_ = [("point", ctypes.c_uint64 * 2), ("ranges", ctypes.POINTER(FriPolyRange)), ("n_ranges", ctypes.c_size_t)]


class BatchPoolInfo(ctypes.Structure):
    _fields_ = [("bytes", ctypes.c_size_t), ("buffers", ctypes.c_size_t), ("hits", ctypes.c_size_t), ("misses", ctypes.c_size_t),
                ("trims", ctypes.c_size_t), ("cap_bytes", ctypes.c_size_t), ("pooled", ctypes.c_int)]


class FriOracleInfo(ctypes.Structure):
    _fields_ = [("num_polys", ctypes.c_uint32), ("blinding", ctypes.c_uint32)]


def _fri_batches(batches):
    """[(point (2,), [(oracle, first, count), ...]), ...] -> (ctypes array of FriBatch, keep-alive list)"""
    arr = (FriBatch * len(batches))()
    keep = []
    for i, (pt, ranges) in enumerate(batches):
        rr = (FriPolyRange * max(1, len(ranges)))()
        for j, (o, f, c) in enumerate(ranges):
            rr[j] = FriPolyRange(o, f, c)
        keep.append(rr)
        arr[i].point[0], arr[i].point[1] = int(pt[0]), int(pt[1])
        arr[i].ranges = ctypes.cast(rr, ctypes.POINTER(FriPolyRange))
        arr[i].n_ranges = len(ranges)
    return arr, keep


BATCH_FROM_COEFFS = 1
_u8pp = ctypes.POINTER(ctypes.POINTER(ctypes.c_uint8))
ABI.update({
    "cp_batch_commit": (ctypes.c_int, [_vp, _u64p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint, _u64p,
                                       ctypes.POINTER(_vp)]),
    "cp_batch_commit_dev": (ctypes.c_int, [_vp, _vp, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint, _vp,
                                           ctypes.POINTER(_vp)]),
    "cp_batch_destroy": (None, [_vp]),
    "cp_batch_pool_stats": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(BatchPoolInfo)]),
    "cp_batch_pool_trim": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_size_t)]),
    "cp_batch_info": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_size_t)] + [ctypes.POINTER(ctypes.c_int)] * 4),
    "cp_batch_cap": (ctypes.c_int, [_vp, _u64p]),
    "cp_batch_eval_ext": (ctypes.c_int, [_vp, ctypes.c_size_t, ctypes.c_size_t, _u64p, _u64p]),
    "cp_batch_lde_rows": (ctypes.c_int, [_vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, _u64p]),
    "cp_batch_leaves": (ctypes.c_int, [_vp, ctypes.c_size_t, ctypes.c_size_t, _u64p]),
    "cp_batch_coeffs": (ctypes.c_int, [_vp, ctypes.c_size_t, ctypes.c_size_t, _u64p]),
    "cp_batch_device_ptrs": (ctypes.c_int, [_vp, ctypes.POINTER(_vp), ctypes.POINTER(_vp)]),
    "cp_fri_prove": (ctypes.c_int, [_vp, ctypes.POINTER(_vp), ctypes.c_size_t, ctypes.POINTER(FriBatch), ctypes.c_size_t,
                                    ctypes.POINTER(FriParams), ctypes.POINTER(ChallengerState), ctypes.c_int, ctypes.c_uint64,
                                    _u8pp, ctypes.POINTER(ctypes.c_size_t)]),
    "cp_fri_verify": (ctypes.c_int, [ctypes.POINTER(FriParams), ctypes.POINTER(FriOracleInfo), ctypes.c_size_t,
                                     ctypes.POINTER(_u64p), ctypes.POINTER(FriBatch), ctypes.c_size_t, ctypes.POINTER(_u64p),
                                     ctypes.POINTER(ChallengerState), ctypes.c_char_p, ctypes.c_size_t]),
    "cp_challenger_observe": (ctypes.c_int, [ctypes.POINTER(ChallengerState), _u64p, ctypes.c_size_t]),
    "cp_challenger_challenges": (ctypes.c_int, [ctypes.POINTER(ChallengerState), _u64p, ctypes.c_size_t]),
})


def batch_pool_stats(device=0):
    """the batch-handle buffer pool of `device` (include/cityprover.h cp_batch_pool_stats) as a dict"""
    info = BatchPoolInfo()
    rc = load_library().cp_batch_pool_stats(device, ctypes.byref(info))
    if rc != 0:
        raise CityProverError(rc, load_library().cp_last_error(None).decode())
    return {f: getattr(info, f) for f, _ in BatchPoolInfo._fields_}


def batch_pool_trim(prover):
    released = ctypes.c_size_t(0)
    prover._check(prover.lib.cp_batch_pool_trim(prover.ctx, ctypes.byref(released)))
    return released.value


class PolyBatch:
    """cp_poly_batch: plonky2 `PolynomialBatch` resident on the device (coefficients, bit-reversed LDE, Merkle tree)."""

    def __init__(self, prover, polys, rate_bits, cap_height, from_coeffs=False, salts=None, device_ptr=None, shape=None):
        self.prover = prover
        h = _vp()
        flags = BATCH_FROM_COEFFS if from_coeffs else 0
        if device_ptr is not None:
            k, n = shape
            sp = None if salts is None else salts
            prover._check(prover.lib.cp_batch_commit_dev(prover.ctx, device_ptr, k, int(n).bit_length() - 1, rate_bits, cap_height,
                                                         flags, sp, ctypes.byref(h)))
        else:
            v = _as_u64(polys)
            k, n = v.shape
            s = None if salts is None else _as_u64(salts)
            prover._check(prover.lib.cp_batch_commit(prover.ctx, _ptr(v), k, int(n).bit_length() - 1, rate_bits, cap_height, flags,
                                                     None if s is None else _ptr(s), ctypes.byref(h)))
        self.handle = h.value
        self.k, self.degree_bits, self.rate_bits, self.cap_height = k, int(n).bit_length() - 1, rate_bits, cap_height
        self.blinding = salts is not None

    def cap(self):
        cap = np.zeros((1 << self.cap_height, 4), np.uint64)
        self.prover._check(self.prover.lib.cp_batch_cap(self.handle, _ptr(cap)))
        return cap

    def eval_ext(self, point, first=0, count=None):
        count = self.k - first if count is None else count
        out = np.zeros((count, 2), np.uint64)
        pt = _as_u64(point)
        self.prover._check(self.prover.lib.cp_batch_eval_ext(self.handle, first, count, _ptr(pt), _ptr(out)))
        return out

    def lde_rows(self, first_index, count, step=1):
        out = np.zeros((count, self.k), np.uint64)
        self.prover._check(self.prover.lib.cp_batch_lde_rows(self.handle, first_index, count, step, _ptr(out)))
        return out

    def leaves(self, first_leaf, count):
        out = np.zeros((count, self.k + (SALT_SIZE if self.blinding else 0)), np.uint64)
        self.prover._check(self.prover.lib.cp_batch_leaves(self.handle, first_leaf, count, _ptr(out)))
        return out

    def coeffs(self, first=0, count=None):
        count = self.k - first if count is None else count
        out = np.zeros((count, 1 << self.degree_bits), np.uint64)
        self.prover._check(self.prover.lib.cp_batch_coeffs(self.handle, first, count, _ptr(out)))
        return out

    def device_ptrs(self):
        c, l = _vp(), _vp()
        self.prover._check(self.prover.lib.cp_batch_device_ptrs(self.handle, ctypes.byref(c), ctypes.byref(l)))
        return c.value, l.value

    def close(self):
        if self.handle:
            self.prover.lib.cp_batch_destroy(self.handle)
            self.handle = None


def fri_prove(prover, oracles, batches, params, challenger, pow_override=None):
    """cp_fri_prove: `PolynomialBatch::prove_openings`. oracles: [PolyBatch]; batches: [(point, [(oracle, first, count)])];
    challenger: ChallengerState (advanced in place). Returns bincode FriProof bytes."""
    hs = (_vp * len(oracles))(*[o.handle for o in oracles])
    arr, keep = _fri_batches(batches)
    out = ctypes.POINTER(ctypes.c_uint8)()
    ln = ctypes.c_size_t()
    prover._check(prover.lib.cp_fri_prove(prover.ctx, hs, len(oracles), arr, len(batches), ctypes.byref(params), ctypes.byref(challenger),
                                          0 if pow_override is None else 1, pow_override or 0, ctypes.byref(out), ctypes.byref(ln)))
    try:
        return ctypes.string_at(out, ln.value)
    finally:
        prover.lib.cp_free(out)


def fri_verify(params, oracle_infos, caps, batches, opened_values, challenger, proof_bytes):
    """cp_fri_verify: `fri_challenges` + `verify_fri_proof`. oracle_infos: [(num_polys, blinding)]; caps: [array (2^cap_height, 4)];
    opened_values: per batch an (n_polys, 2) array. Raises CityProverError on rejection; advances `challenger` on success."""
    lib = load_library()
    infos = (FriOracleInfo * len(oracle_infos))(*[FriOracleInfo(int(k), int(bool(b))) for k, b in oracle_infos])
    cap_arrs = [_as_u64(c) for c in caps]
    capp = (_u64p * len(cap_arrs))(*[_ptr(c) for c in cap_arrs])
    arr, keep = _fri_batches(batches)
    ov = [_as_u64(o) for o in opened_values]
    ovp = (_u64p * len(ov))(*[_ptr(o) if o.size else None for o in ov])
    rc = lib.cp_fri_verify(ctypes.byref(params), infos, len(oracle_infos), capp, arr, len(batches), ovp, ctypes.byref(challenger),
                           proof_bytes, len(proof_bytes))
    if rc != 0:
        raise CityProverError(f"[{rc}] " + lib.cp_last_error(None).decode())


# ---- generic AIR machinery (include/cityprover.h "the STARK's own two steps as GENERIC device machinery") -----------------
(AIR_LOCAL, AIR_NEXT, AIR_PUBLIC, AIR_GLOBAL, AIR_CHALLENGE, AIR_CONST, AIR_ADD, AIR_SUB, AIR_MUL, AIR_NEG, AIR_INV, AIR_ASSERT_ZERO,
 AIR_ASSERT_ZERO_TRANSITION, AIR_ASSERT_ZERO_FIRST_ROW, AIR_ASSERT_ZERO_LAST_ROW, AIR_STORE) = range(16)
AIR_CONSTRAINTS, AIR_MAP = 0, 1
STARK_STEP_MAP, STARK_STEP_CUBIC_INVERSE, STARK_STEP_PREFIX_SUM = 0, 1, 2


class AirProgramDesc(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int), ("ops", _vp), ("n_ops", ctypes.c_size_t), ("consts", _u64p), ("n_consts", ctypes.c_size_t),
                ("n_columns", ctypes.c_uint32), ("n_public", ctypes.c_uint32), ("n_global", ctypes.c_uint32), ("n_challenge", ctypes.c_uint32),
                ("n_out_columns", ctypes.c_uint32)]


class AirProgramInfo(ctypes.Structure):
    _fields_ = [("n_ops", ctypes.c_size_t), ("n_live_ops", ctypes.c_size_t), ("n_constraints", ctypes.c_size_t),
                ("max_constraint_degree", ctypes.c_uint32), ("n_segments_max", ctypes.c_uint32), ("n_slots", ctypes.c_uint32),
                ("n_instructions", ctypes.c_size_t)]


class StarkStep(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int), ("program", _vp), ("first", ctypes.c_uint32), ("count", ctypes.c_uint32), ("flags", ctypes.c_uint32),
                ("modulus", ctypes.c_uint64 * 2)]


class StarkDesc(ctypes.Structure):
    _fields_ = [("degree_bits", ctypes.c_int), ("quotient_degree_bits", ctypes.c_int), ("num_challenges", ctypes.c_uint32), ("fri", FriParams),
                ("n_trace_columns", ctypes.c_uint32), ("n_extended_columns", ctypes.c_uint32), ("n_round_challenges", ctypes.c_uint32),
                ("n_public", ctypes.c_uint32), ("n_global", ctypes.c_uint32), ("steps", ctypes.POINTER(StarkStep)), ("n_steps", ctypes.c_size_t),
                ("constraints", _vp)]


ABI.update({
    "cp_air_program_create": (_vp, [_vp, ctypes.POINTER(AirProgramDesc)]),
    "cp_air_program_destroy": (None, [_vp]),
    "cp_air_program_get_info": (ctypes.c_int, [_vp, ctypes.POINTER(AirProgramInfo)]),
    "cp_air_program_eval_ext": (ctypes.c_int, [_vp, _u64p, _u64p, _u64p, _u64p, _u64p, _u64p, ctypes.POINTER(ctypes.c_uint32)]),
    "cp_air_quotient_commit": (ctypes.c_int, [_vp, _vp, ctypes.POINTER(_vp), ctypes.c_size_t, ctypes.c_int, _u64p, _u64p, _u64p, _u64p,
                                              ctypes.c_size_t, ctypes.POINTER(_vp)]),
    "cp_air_map_dev": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_size_t, _u64p, _u64p, _u64p]),
    "cp_cubic_batch_inverse_dev": (ctypes.c_int, [_vp, _u64p, _vp, ctypes.c_size_t, ctypes.c_size_t]),
    "cp_column_prefix_sum_dev": (ctypes.c_int, [_vp, _vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int]),
    "cp_stark_prove": (ctypes.c_int, [_vp, ctypes.POINTER(StarkDesc), _vp, ctypes.c_int, _u64p, _u64p, ctypes.POINTER(ChallengerState), ctypes.c_int,
                                      ctypes.c_uint64, _u8pp, ctypes.POINTER(ctypes.c_size_t)]),
    "cp_stark_prove_batch": (ctypes.c_int, [_vp, ctypes.POINTER(StarkDesc), ctypes.c_size_t, ctypes.POINTER(_vp), ctypes.c_int, _u64p, _u64p,
                                            ctypes.POINTER(ChallengerState), ctypes.POINTER(ctypes.c_int), _u64p, _u8pp, ctypes.POINTER(ctypes.c_size_t)]),
    "cp_stark_verify": (ctypes.c_int, [ctypes.POINTER(StarkDesc), _u64p, _u64p, ctypes.POINTER(ChallengerState), ctypes.c_char_p, ctypes.c_size_t]),
    "cp_stark_verify_batch": (ctypes.c_int, [_vp, ctypes.POINTER(StarkDesc), ctypes.c_size_t, _u64p, _u64p, ctypes.POINTER(ChallengerState),
                                             ctypes.POINTER(ctypes.c_char_p), _szp, ctypes.c_size_t, ctypes.c_uint, _vp]),
})
STARK_BATCH_MAX = 64
# path_form of cp_stark_verify_batch: which kernel checks the Merkle paths
PATHS_AUTO, PATHS_LANE, PATHS_COOP = 0, 1, 2


def _opt_u64(x):
    """None / empty -> (NULL, keep-alive None); else a contiguous u64 array and its pointer"""
    if x is None:
        return None, None
    a = _as_u64(x)
    return (_ptr(a) if a.size else None), a


class AirProgram:
    """cp_air_program: a straight-line program over F_p. ops: (n, 4) uint32 rows (op, a, b, 0) with the AIR_* codes."""

    def __init__(self, prover, kind, ops, consts=(), n_columns=0, n_public=0, n_global=0, n_challenge=0, n_out_columns=0):
        self.prover = prover
        o = np.ascontiguousarray(np.asarray(ops, dtype=np.uint32).reshape(-1, 4))
        c = _as_u64(np.asarray(list(consts) if not isinstance(consts, np.ndarray) else consts, dtype=np.uint64))
        d = AirProgramDesc(kind, o.ctypes.data if o.size else None, len(o), _ptr(c) if c.size else None, c.size, n_columns, n_public, n_global,
                           n_challenge, n_out_columns)
        self.handle = prover.lib.cp_air_program_create(prover.ctx, ctypes.byref(d))
        if not self.handle:
            raise CityProverError(prover.lib.cp_last_error(prover.ctx).decode())
        self.kind, self.n_columns, self.n_public, self.n_global, self.n_challenge, self.n_out_columns = kind, n_columns, n_public, n_global, n_challenge, n_out_columns

    def info(self):
        i = AirProgramInfo()
        self.prover._check(self.prover.lib.cp_air_program_get_info(self.handle, ctypes.byref(i)))
        return {f: getattr(i, f) for f, _ in AirProgramInfo._fields_}

    def eval_ext(self, local, nxt, publics=None, globals_=None, challenges=None):
        """constraint values on one row over F_p^2: ((n_constraints, 2) array, kinds)"""
        n = self.info()["n_constraints"]
        out = np.zeros((n, 2), np.uint64)
        kinds = np.zeros(max(n, 1), np.uint32)
        ptrs, keep = zip(*[_opt_u64(x) for x in (local, nxt, publics, globals_, challenges)])
        self.prover._check(self.prover.lib.cp_air_program_eval_ext(self.handle, *ptrs, _ptr(out), kinds.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))))
        return out, kinds[:n]

    def close(self):
        if self.handle:
            self.prover.lib.cp_air_program_destroy(self.handle)
            self.handle = None


def _wrap_batch(prover, handle):
    b = PolyBatch.__new__(PolyBatch)
    b.prover, b.handle = prover, handle
    k, db, rb, ch, ns = ctypes.c_size_t(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    prover._check(prover.lib.cp_batch_info(handle, ctypes.byref(k), ctypes.byref(db), ctypes.byref(rb), ctypes.byref(ch), ctypes.byref(ns)))
    b.k, b.degree_bits, b.rate_bits, b.cap_height, b.blinding = k.value, db.value, rb.value, ch.value, ns.value != 0
    return b


def air_quotient_commit(prover, program, oracles, quotient_degree_bits, alphas, publics=None, globals_=None, challenges=None):
    """cp_air_quotient_commit -> PolyBatch of len(alphas) * 2^q quotient chunk polynomials"""
    hs = (_vp * len(oracles))(*[o.handle for o in oracles])
    al = _as_u64(alphas)
    (pp, gp, cp_), keep = zip(*[_opt_u64(x) for x in (publics, globals_, challenges)])
    out = _vp()
    prover._check(prover.lib.cp_air_quotient_commit(prover.ctx, program.handle, hs, len(oracles), quotient_degree_bits, pp, gp, cp_, _ptr(al), al.size,
                                                    ctypes.byref(out)))
    return _wrap_batch(prover, out.value)


def air_map(prover, program, in_cols, publics=None, globals_=None, challenges=None):
    """cp_air_map_dev on host arrays: in_cols (n_columns, n) -> (n_out_columns, n) (columns never stored stay 0)"""
    v = _as_u64(in_cols)
    n = v.shape[1]
    din = prover.to_device(v)
    dout = prover.alloc(max(program.n_out_columns, 1) * n)
    try:
        dout.upload(np.zeros(max(program.n_out_columns, 1) * n, np.uint64))
        (pp, gp, cp_), keep = zip(*[_opt_u64(x) for x in (publics, globals_, challenges)])
        prover._check(prover.lib.cp_air_map_dev(prover.ctx, program.handle, din.ptr, dout.ptr, n, pp, gp, cp_))
        return dout.download(program.n_out_columns * n).reshape(program.n_out_columns, n)
    finally:
        din.free()
        dout.free()


def cubic_batch_inverse(prover, modulus, cols):
    """cp_cubic_batch_inverse_dev on a host array: cols (3 * count, n) -> the inverses, same layout"""
    v = _as_u64(cols)
    d = prover.to_device(v)
    try:
        m = _as_u64(modulus)
        prover._check(prover.lib.cp_cubic_batch_inverse_dev(prover.ctx, _ptr(m), d.ptr, v.shape[0] // 3, v.shape[1]))
        return d.download(v.size).reshape(v.shape)
    finally:
        d.free()


def column_prefix_sum(prover, cols, exclusive=False):
    v = _as_u64(cols)
    d = prover.to_device(v)
    try:
        prover._check(prover.lib.cp_column_prefix_sum_dev(prover.ctx, d.ptr, v.shape[0], v.shape[1], int(exclusive)))
        return d.download(v.size).reshape(v.shape)
    finally:
        d.free()


def stark_desc(degree_bits, quotient_degree_bits, num_challenges, fri, n_trace_columns, constraints, n_extended_columns=0, n_round_challenges=0,
               n_public=0, n_global=0, steps=()):
    """cp_stark_desc. steps: [("map", AirProgram) | ("cubic_inverse", first, count, (m0, m1)) | ("prefix_sum", first, count, exclusive)].
    Returns (desc, keep-alive) — hold on to both."""
    arr = (StarkStep * max(1, len(steps)))()
    for i, st in enumerate(steps):
        if st[0] == "map":
            arr[i].kind, arr[i].program = STARK_STEP_MAP, st[1].handle
        elif st[0] == "cubic_inverse":
            arr[i].kind, arr[i].first, arr[i].count = STARK_STEP_CUBIC_INVERSE, st[1], st[2]
            arr[i].modulus[0], arr[i].modulus[1] = int(st[3][0]), int(st[3][1])
        elif st[0] == "prefix_sum":
            arr[i].kind, arr[i].first, arr[i].count, arr[i].flags = STARK_STEP_PREFIX_SUM, st[1], st[2], int(bool(st[3]))
        else:
            raise ValueError(st[0])
    d = StarkDesc(degree_bits, quotient_degree_bits, num_challenges, fri, n_trace_columns, n_extended_columns, n_round_challenges, n_public, n_global,
                  ctypes.cast(arr, ctypes.POINTER(StarkStep)), len(steps), constraints.handle)
    return d, (arr, steps, constraints)


def stark_prove(prover, desc, trace, challenger, publics=None, globals_=None, pow_override=None):
    """cp_stark_prove: trace (n_trace_columns, n) host array -> proof bytes; advances `challenger`"""
    t = _as_u64(trace)
    (pp, gp), keep = zip(*[_opt_u64(x) for x in (publics, globals_)])
    out, ln = ctypes.POINTER(ctypes.c_uint8)(), ctypes.c_size_t(0)
    prover._check(prover.lib.cp_stark_prove(prover.ctx, ctypes.byref(desc), t.ctypes.data, 0, pp, gp, ctypes.byref(challenger),
                                            0 if pow_override is None else 1, 0 if pow_override is None else int(pow_override),
                                            ctypes.byref(out), ctypes.byref(ln)))
    try:
        return ctypes.string_at(out, ln.value)
    finally:
        prover.lib.cp_free(out)


def stark_prove_batch(prover, desc, traces, challengers, publics=None, globals_=None, pow_overrides=None):
    """cp_stark_prove_batch: traces = B host arrays (n_trace_columns, n) of ONE description -> list of B proof bytes, instance i the
    bytes stark_prove gives for traces[i] and challengers[i] alone. publics / globals_: (B, n_public) / (B, n_global) or None;
    pow_overrides: B entries, None = search a witness. Advances every ChallengerState in place; on an error none has moved."""
    B = len(traces)
    if len(challengers) != B or (pow_overrides is not None and len(pow_overrides) != B):
        raise ValueError("one challenger (and one pow override entry) per trace")
    ts = [_as_u64(t) for t in traces]
    tp = (_vp * max(B, 1))(*[t.ctypes.data for t in ts])
    (pp, gp), keep = zip(*[_opt_u64(x) for x in (publics, globals_)])
    ch = (ChallengerState * max(B, 1))()
    for i, c in enumerate(challengers):
        ctypes.memmove(ctypes.byref(ch[i]), ctypes.byref(c), ctypes.sizeof(ChallengerState))
    up = ov = None
    if pow_overrides is not None:
        up = (ctypes.c_int * max(B, 1))(*[0 if w is None else 1 for w in pow_overrides])
        ov = (ctypes.c_uint64 * max(B, 1))(*[0 if w is None else int(w) for w in pow_overrides])
    outs, lens = (ctypes.POINTER(ctypes.c_uint8) * max(B, 1))(), (ctypes.c_size_t * max(B, 1))()
    prover._check(prover.lib.cp_stark_prove_batch(prover.ctx, ctypes.byref(desc), B, tp, 0, pp, gp, ch, up, ov, outs, lens))
    try:
        proofs = [ctypes.string_at(outs[i], lens[i]) for i in range(B)]
    finally:
        for i in range(B):
            prover.lib.cp_free(outs[i])
    for i, c in enumerate(challengers):
        ctypes.memmove(ctypes.byref(c), ctypes.byref(ch[i]), ctypes.sizeof(ChallengerState))
    return proofs


def stark_verify(desc, challenger, proof, publics=None, globals_=None):
    lib = load_library()
    (pp, gp), keep = zip(*[_opt_u64(x) for x in (publics, globals_)])
    rc = lib.cp_stark_verify(ctypes.byref(desc), pp, gp, ctypes.byref(challenger), proof, len(proof))
    if rc != 0:
        raise CityProverError(f"[{rc}] " + lib.cp_last_error(None).decode())


def stark_verify_batch(prover, desc, challengers, proofs, publics=None, globals_=None, chunk=0, path_form=PATHS_AUTO):
    """cp_stark_verify_batch: B proofs of ONE description -> list of B (status, query, detail), the statuses of VERDICT. publics /
    globals_: (B, n_public) / (B, n_global) or None. The ChallengerState of every ACCEPTED proof is advanced in place as stark_verify
    advances it; a rejected proof's stays as it came in. Raises only for a call that could not run (then nothing has moved)."""
    keep, ptrs, lens = _proof_array(proofs)
    B = len(keep)
    if len(challengers) != B:
        raise ValueError("one challenger per proof")
    (pp, gp), keep2 = zip(*[_opt_u64(x) for x in (publics, globals_)])
    ch = (ChallengerState * max(B, 1))()
    for i, c in enumerate(challengers):
        ctypes.memmove(ctypes.byref(ch[i]), ctypes.byref(c), ctypes.sizeof(ChallengerState))
    out = np.zeros(max(B, 1), VERDICT)
    prover._check(prover.lib.cp_stark_verify_batch(prover.ctx, ctypes.byref(desc), B, pp, gp, ch, ptrs, lens, int(chunk), int(path_form), out.ctypes.data))
    for i, c in enumerate(challengers):
        ctypes.memmove(ctypes.byref(c), ctypes.byref(ch[i]), ctypes.sizeof(ChallengerState))
    return [(int(v["status"]), int(v["query"]), int(v["detail"])) for v in out[:B]]


# ---- does the witness satisfy the circuit, and where not? (include/cityprover.h; INTEGRATION.md "When a proof does not verify") ----
class WitnessReport(ctypes.Structure):
    """cp_witness_report"""
    _fields_ = [("n_gate_violations", ctypes.c_uint64), ("n_copy_violations", ctypes.c_uint64), ("n_sigma_undecodable", ctypes.c_uint64),
                ("n_noncanonical", ctypes.c_uint64), ("gate_row", ctypes.c_int64), ("gate_index", ctypes.c_int32), ("gate_type", ctypes.c_int32),
                ("constraint", ctypes.c_int32), ("constraint_value", ctypes.c_uint64), ("copy_row", ctypes.c_int64), ("copy_column", ctypes.c_int32),
                ("copy_to_row", ctypes.c_int64), ("copy_to_column", ctypes.c_int32), ("copy_value", ctypes.c_uint64), ("copy_to_value", ctypes.c_uint64),
                ("sigma_row", ctypes.c_int64), ("sigma_column", ctypes.c_int32), ("noncanonical_row", ctypes.c_int64),
                ("noncanonical_column", ctypes.c_int32)]


class AirCheckReport(ctypes.Structure):
    """cp_air_check_report"""
    _fields_ = [("n_violations", ctypes.c_uint64), ("row", ctypes.c_int64), ("sink", ctypes.c_int64), ("sink_kind", ctypes.c_int32),
                ("value", ctypes.c_uint64)]


ABI["cp_circuit_check_witness_dev"] = (ctypes.c_int, [_vp, ctypes.c_size_t, ctypes.POINTER(_vp), ctypes.POINTER(_u64p), ctypes.POINTER(ctypes.c_size_t),
                                                      _vp, ctypes.POINTER(WitnessReport), _u64p])
ABI["cp_circuit_check_witness"] = (ctypes.c_int, [_vp, _u64p, _u64p, ctypes.c_size_t, ctypes.POINTER(WitnessReport), _u64p])
ABI["cp_air_check_rows_dev"] = (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_size_t, _u64p, _u64p, _u64p, ctypes.POINTER(AirCheckReport), _u64p])
ABI["cp_stark_check_trace"] = (ctypes.c_int, [_vp, ctypes.POINTER(StarkDesc), _vp, ctypes.c_int, _u64p, _u64p, _u64p, ctypes.POINTER(AirCheckReport), _u64p])


def _report_dict(r, extra):
    d = {f: int(getattr(r, f)) for f, _ in r._fields_}
    d.update(extra)
    return d


def check_witness_batch_dev(prover, circuits, public_inputs, wires_ptr):
    """cp_circuit_check_witness_dev: wires_ptr = device [proof][num_wires][n], arguments as prove_batch_dev. One dict per witness: the
    fields of cp_witness_report, and "per_gate" = the count of violated (row, constraint) pairs of every gate index."""
    B = len(circuits)
    cs = (_vp * max(B, 1))(*[c.handle for c in circuits])
    pis = [_as_u64(p) for p in public_inputs]
    pi_ptrs = (_u64p * max(B, 1))(*[_ptr(p) if p.size else None for p in pis])
    n_pis = (ctypes.c_size_t * max(B, 1))(*[p.size for p in pis])
    reports = (WitnessReport * max(B, 1))()
    per_gate = np.zeros((max(B, 1), 32), np.uint64)   # at most 32 gates per circuit; the library writes n_proofs x n_gates
    prover._check(prover.lib.cp_circuit_check_witness_dev(prover.ctx, B, cs, pi_ptrs, n_pis, wires_ptr, reports, _ptr(per_gate)))
    ng = getattr(circuits[0], "n_gates", None)   # None: the gate list was set behind this binding's back
    flat = per_gate.reshape(-1)
    out = []
    for i in range(B):
        pg = [int(v) for v in flat[i * ng:(i + 1) * ng]] if ng is not None else None
        out.append(_report_dict(reports[i], {"per_gate": pg}))
    return out


def check_witness(circuit, wires, public_inputs):
    """cp_circuit_check_witness: one witness [num_wires][n] in host memory -> the dict of check_witness_batch_dev"""
    pr = circuit.prover
    w, pi = _as_u64(wires), _as_u64(public_inputs)
    if w.size != circuit.shape.num_wires << circuit.shape.degree_bits:
        raise ValueError("wires must be [num_wires][n]")
    r = WitnessReport()
    per_gate = np.zeros(32, np.uint64)
    pr._check(pr.lib.cp_circuit_check_witness(circuit.handle, _ptr(w), _ptr(pi) if pi.size else None, pi.size, ctypes.byref(r), _ptr(per_gate)))
    ng = getattr(circuit, "n_gates", None)
    return _report_dict(r, {"per_gate": [int(v) for v in per_gate[:ng]] if ng is not None else None})


def _air_check_result(r, per_sink):
    return _report_dict(r, {"per_sink": [int(v) for v in per_sink]})


def _air_check_rows(self, cols, publics=None, globals_=None, challenges=None):
    """cp_air_check_rows_dev on a host array: cols (n_columns, n) in natural row order -> the fields of cp_air_check_report and
    "per_sink" = the number of violated rows of every sink"""
    v = _as_u64(cols)
    n = v.shape[1]
    d = self.prover.to_device(v)
    try:
        return self.check_rows_dev(d.ptr, n, publics, globals_, challenges)
    finally:
        d.free()


def _air_check_rows_dev(self, cols_ptr, n, publics=None, globals_=None, challenges=None):
    (pp, gp, cp_), keep = zip(*[_opt_u64(x) for x in (publics, globals_, challenges)])
    r = AirCheckReport()
    per_sink = np.zeros(max(self.info()["n_constraints"], 1), np.uint64)
    self.prover._check(self.prover.lib.cp_air_check_rows_dev(self.prover.ctx, self.handle, cols_ptr, n, pp, gp, cp_, ctypes.byref(r), _ptr(per_sink)))
    return _air_check_result(r, per_sink[:self.info()["n_constraints"]])


AirProgram.check_rows = _air_check_rows
AirProgram.check_rows_dev = _air_check_rows_dev


def stark_check_trace(prover, desc, trace, publics=None, globals_=None, round_challenges=None, n_constraints=None):
    """cp_stark_check_trace: trace (n_trace_columns, n) host array; the extended columns are filled under round_challenges. n_constraints:
    the number of sinks of desc.constraints, for "per_sink" (None: not returned)."""
    t = _as_u64(trace)
    (pp, gp, rp), keep = zip(*[_opt_u64(x) for x in (publics, globals_, round_challenges)])
    r = AirCheckReport()
    per_sink = np.zeros(max(n_constraints or 0, 1), np.uint64)
    prover._check(prover.lib.cp_stark_check_trace(prover.ctx, ctypes.byref(desc), t.ctypes.data, 0, pp, gp, rp, ctypes.byref(r),
                                                  _ptr(per_sink) if n_constraints is not None else None))
    return _air_check_result(r, per_sink[:n_constraints or 0])
