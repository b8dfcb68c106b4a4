"""ctypes binding of libjolt_hip.so (include/jolt_hip.h) -- the same C ABI a Rust FFI crate would bind.

Field elements are numpy uint64 arrays of shape (..., 4) (Montgomery limbs of jolt_field::Fr); G1 points are
(..., 12) uint64 (Jacobian, ark_bn254::G1Projective layout).  There is no CPU fallback: if the shared library is
missing or no gfx950 device is usable, the calls raise.
"""
import ctypes as C
import os

import numpy as np

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libjolt_hip.so")

STATUS = {abi.CONSTANTS[name]: text for name, text in {
    "JOLT_OK": "ok", "JOLT_ERR_INVALID_ARG": "invalid argument", "JOLT_ERR_NO_DEVICE": "no device", "JOLT_ERR_OOM": "oom", "JOLT_ERR_HIP": "hip error",
    "JOLT_ERR_SIZE_MISMATCH": "size mismatch", "JOLT_ERR_UNSUPPORTED": "unsupported", "JOLT_ERR_NOT_FULLY_BOUND": "not fully bound", "JOLT_ERR_ROUND_CHECK": "round check failed",
    "JOLT_ERR_SRS_TOO_SMALL": "srs too small", "JOLT_ERR_EMPTY_POINT": "empty point", "JOLT_ERR_NOT_INVERTIBLE": "not invertible"}.items()}
# every constant of the header under its name without the JOLT_ prefix: ORDER_LOW_TO_HIGH, MEMBER_FLAG_SKIP_ONE, PAIRING_LINES, DORY_KIND_G1, ...
# (but the transcript kinds: TRANSCRIPT_* below are the kinds shifted into a label's top bits)
globals().update({name[len("JOLT_"):]: value for name, value in abi.CONSTANTS.items() if not name.startswith("JOLT_TRANSCRIPT_")})


class JoltError(RuntimeError):
    def __init__(self, status, where, detail=""):
        self.status = status
        super().__init__(f"{where}: status {status} ({STATUS.get(status, '?')}) {detail}")


class MemberDesc(C.Structure):
    _fields_ = [("n_tables", C.c_uint32), ("n_terms", C.c_uint32), ("degree", C.c_uint32), ("order", C.c_int32),
                ("term_offsets", C.c_void_p), ("factors", C.c_void_p), ("coeffs", C.c_void_p)]


class MemberLcDesc(C.Structure):
    _fields_ = [("n_tables", C.c_uint32), ("n_groups", C.c_uint32), ("n_factors", C.c_uint32), ("n_lc", C.c_uint32),
                ("degree", C.c_uint32), ("order", C.c_int32), ("flags", C.c_uint32),
                ("group_factor_offsets", C.c_void_p), ("factor_lc_offsets", C.c_void_p), ("factor_consts", C.c_void_p),
                ("lc_tables", C.c_void_p), ("lc_coeffs", C.c_void_p)]


_lib = None


def lib():
    """Load the native library (fails loudly when it has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: run `python -m jolt_amd.build` (there is no CPU fallback)")
        os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")  # (capi.hip sets the same default when the library is loaded; here for processes whose HIP runtime starts before it)
        loaded = C.CDLL(LIB_PATH)
        abi.declare(loaded)  # every entry point gets the header's prototype: call sites pass plain ints, a mistyped argument is a ctypes.ArgumentError
        _lib = loaded
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def fr(a):
    return np.ascontiguousarray(a, dtype=np.uint64)


def fr_array(n):
    return np.zeros((n, 4), dtype=np.uint64)


def g1_array(n):
    return np.zeros((n, 12), dtype=np.uint64)


def _ck(status, where, ctx=None):
    if status != 0:
        detail = ""
        if ctx is not None and ctx.h:
            detail = lib().jolt_last_error(ctx.h).decode()
        raise JoltError(status, where, detail)


def _call(name, ctx, *args):
    """call entry point `name` and raise JoltError (with ctx's last error text) unless it returns JOLT_OK"""
    _ck(getattr(lib(), name)(*args), name, ctx)


class Context:
    def __init__(self, device_id=0, stream=None):
        self.h = C.c_void_p()
        self.device_id = device_id
        st = lib().jolt_ctx_create(device_id, C.c_void_p(stream) if stream else None, C.byref(self.h))
        if st != 0:
            self.h = C.c_void_p()
            raise JoltError(st, "jolt_ctx_create")

    def close(self):
        if self.h:
            lib().jolt_ctx_destroy(self.h)
            self.h = C.c_void_p()

    def bind_thread(self):
        """select this context's device on the calling thread (a worker thread starts on device 0)"""
        _call("jolt_ctx_bind_thread", self, self.h)

    def synchronize_foreground(self):
        """every stream but the background one (the opening hint's class sums)"""
        _call("jolt_ctx_synchronize_foreground", self, self.h)

    def synchronize(self):
        _call("jolt_ctx_synchronize", self, self.h)

    def timer_begin(self):
        _call("jolt_timer_begin", self, self.h)

    def timer_end(self):
        ms = C.c_float()
        _call("jolt_timer_end", self, self.h, C.byref(ms))
        return ms.value

    # ---- tables
    def upload(self, arr):
        a = fr(arr).reshape(-1, 4)
        h = C.c_void_p()
        _call("jolt_table_upload", self, self.h, _p(a), a.shape[0], C.byref(h))
        return Table(self, h)

    def from_device(self, ptr, length):
        h = C.c_void_p()
        _call("jolt_table_from_device", self, self.h, C.c_void_p(ptr), length, C.byref(h))
        return Table(self, h)

    def alloc(self, length):
        h = C.c_void_p()
        _call("jolt_table_alloc", self, self.h, length, C.byref(h))
        return Table(self, h)

    def from_u64(self, vals):
        v = np.ascontiguousarray(vals, dtype=np.uint64)
        h = C.c_void_p()
        _call("jolt_table_from_u64", self, self.h, _p(v), v.shape[0], C.byref(h))
        return Table(self, h)

    def from_i64(self, vals):
        v = np.ascontiguousarray(vals, dtype=np.int64)
        h = C.c_void_p()
        _call("jolt_table_from_i64", self, self.h, _p(v), v.shape[0], C.byref(h))
        return Table(self, h)

    def bind(self, tables, r, order=ORDER_LOW_TO_HIGH):
        hs = (C.c_void_p * len(tables))(*[t.h for t in tables])
        _call("jolt_bind", self, self.h, hs, len(tables), _p(fr(r)), order)

    def eq_evals(self, r, scale=None):
        r = fr(r).reshape(-1, 4)
        h = C.c_void_p()
        _call("jolt_eq_evals", self, self.h, _p(r), r.shape[0], _p(fr(scale)) if scale is not None else None, C.byref(h))
        return Table(self, h)

    def eq_evals_aligned_block(self, r, start, block):
        r = fr(r).reshape(-1, 4)
        h = C.c_void_p()
        _call("jolt_eq_evals_aligned_block", self, self.h, _p(r), r.shape[0], start, block, C.byref(h))
        return Table(self, h)

    def lt_evals(self, r):
        r = fr(r).reshape(-1, 4)
        h = C.c_void_p()
        _call("jolt_lt_evals", self, self.h, _p(r), r.shape[0], C.byref(h))
        return Table(self, h)

    def eq_plus_one_evals(self, r, scale=None):
        r = fr(r).reshape(-1, 4)
        h1, h2 = C.c_void_p(), C.c_void_p()
        _call("jolt_eq_plus_one_evals", self, self.h, _p(r), r.shape[0], _p(fr(scale)) if scale is not None else None, C.byref(h1), C.byref(h2))
        return Table(self, h1), Table(self, h2)

    def evaluate(self, table, point):
        p = fr(point).reshape(-1, 4)
        o = fr_array(1)
        _call("jolt_table_evaluate", self, self.h, table.h, _p(p), p.shape[0], _p(o))
        return o[0]

    def table_sum(self, table):
        o = fr_array(1)
        _call("jolt_table_sum", self, self.h, table.h, _p(o))
        return o[0]

    # ---- members
    def member_expr(self, tables, terms, degree, order=ORDER_LOW_TO_HIGH):
        """terms = [(coeff_limbs, [table indices]), ...]; takes ownership of the tables."""
        offs, facs = [0], []
        for _, f in terms:
            facs.extend(f)
            offs.append(len(facs))
        offs = np.array(offs, dtype=np.uint32)
        facs_a = np.array(facs if facs else [0], dtype=np.uint32)
        coeffs = np.ascontiguousarray(np.stack([fr(c) for c, _ in terms])).reshape(-1, 4)
        d = MemberDesc(len(tables), len(terms), degree, order, offs.ctypes.data, facs_a.ctypes.data, coeffs.ctypes.data)
        hs = (C.c_void_p * len(tables))(*[t.h for t in tables])
        h = C.c_void_p()
        _call("jolt_member_create_expr", self, self.h, hs, C.byref(d), C.byref(h))
        for t in tables:
            t.h = None  # ownership moved into the member
        return Member(self, h, degree, len(tables), False, False)

    def member_lc(self, tables, groups, degree, order=ORDER_LOW_TO_HIGH, skip_one=False, borrow=False, eq_point=None, eq_scale=None,
                  shard_scale=None):
        """groups = [[factor, ...], ...]; factor = (const_limbs_or_None, [(coeff_limbs, table_idx), ...]).
        borrow=True: the member only reads `tables` (caller keeps ownership, tables must outlive the member).
        eq_point: the summand is eq(eq_point, j) * (these groups) with the eq weight factored out (jolt_member_create_split_eq_lc);
        `degree` is then the inner degree and prove_round returns q(0), q(2), .., q(degree)."""
        goff, foff, consts, ltab, lcoef = [0], [0], [], [], []
        zero = np.zeros(4, dtype=np.uint64)
        for g in groups:
            for const, entries in g:
                consts.append(zero if const is None else fr(const))
                for c, ti in entries:
                    lcoef.append(fr(c))
                    ltab.append(ti)
                foff.append(len(ltab))
            goff.append(len(consts))
        goff = np.array(goff, dtype=np.uint32)
        foff = np.array(foff, dtype=np.uint32)
        consts_a = np.ascontiguousarray(np.stack(consts)) if consts else fr_array(1)
        ltab_a = np.array(ltab if ltab else [0], dtype=np.uint32)
        lcoef_a = np.ascontiguousarray(np.stack(lcoef)) if lcoef else fr_array(1)
        flags = (MEMBER_FLAG_SKIP_ONE if skip_one else 0) | (MEMBER_FLAG_BORROW_TABLES if borrow else 0)
        d = MemberLcDesc(len(tables), len(groups), len(consts), len(ltab), degree, order, flags,
                         goff.ctypes.data, foff.ctypes.data, consts_a.ctypes.data, ltab_a.ctypes.data, lcoef_a.ctypes.data)
        small = any(isinstance(t, Ints) for t in tables)  # compact-scalar slots: resident u64 columns read unpromoted in round 0 (jolt_member_create_lc_small)
        hs = (C.c_void_p * len(tables))(*[None if isinstance(t, Ints) else t.h for t in tables])
        h = C.c_void_p()
        if small:
            assert borrow and order == ORDER_LOW_TO_HIGH, "integer-backed slots: borrowed tables, LowToHigh"
            ih = (C.c_void_p * len(tables))(*[t.h if isinstance(t, Ints) else None for t in tables])
            w = fr(eq_point).reshape(-1, 4) if eq_point is not None else None
            _call("jolt_member_create_lc_small", self, self.h, hs, ih, C.byref(d), _p(w) if w is not None else None, 0 if w is None else w.shape[0],
                  _p(fr(eq_scale)) if eq_scale is not None else None, _p(fr(shard_scale)) if shard_scale is not None else None, C.byref(h))
            if eq_point is not None:
                m = Member(self, h, degree + 1, len(tables), True, True)
                m.n_evals = degree
                m.uniform = True
                m.eq_weighted = True
            else:
                m = Member(self, h, degree, len(tables), False, skip_one)
        elif eq_point is not None:
            w = fr(eq_point).reshape(-1, 4)
            _call("jolt_member_create_split_eq_lc", self, self.h, hs, C.byref(d), _p(w), w.shape[0], _p(fr(eq_scale)) if eq_scale is not None else None,
                  _p(fr(shard_scale)) if shard_scale is not None else None, C.byref(h))
            m = Member(self, h, degree + 1, len(tables), True, True)
            m.n_evals = degree
            m.uniform = True  # same host-side shape as the uniform member: dq sums, gruen_poly_from_q
            m.eq_weighted = True
        else:
            _call("jolt_member_create_lc", self, self.h, hs, C.byref(d), C.byref(h))
            m = Member(self, h, degree, len(tables), False, skip_one)
        if borrow:
            m._keepalive = list(tables)
        else:
            for t in tables:
                t.h = None
        return m

    def member_split_eq_product(self, a, b, w, scale=None, borrow=False):
        w = fr(w).reshape(-1, 4)
        h = C.c_void_p()
        fn = lib().jolt_member_create_split_eq_product_borrowed if borrow else lib().jolt_member_create_split_eq_product
        _ck(fn(self.h, a.h, b.h, _p(w), w.shape[0], _p(fr(scale)) if scale is not None else None, C.byref(h)),
            "jolt_member_create_split_eq_product", self)
        m = Member(self, h, 3, 2, True, False)
        if borrow:
            m._keepalive = [a, b]
        else:
            a.h = None
            b.h = None
        return m

    def member_split_eq_product_sharded(self, a, b, w_local, scale=None, shard_scale=None):
        """one rank's shard of the split-eq product member (jolt_member_create_split_eq_product_sharded): a, b hold the rank's block of rows (borrowed), w_local the
        low log2(rows) coordinates of the point, shard_scale = eq(w_hi, rank)"""
        w = fr(w_local).reshape(-1, 4)
        h = C.c_void_p()
        _call("jolt_member_create_split_eq_product_sharded", self, self.h, a.h, b.h, _p(w), w.shape[0], _p(fr(scale)) if scale is not None else None,
              _p(fr(shard_scale)) if shard_scale is not None else None, C.byref(h))
        m = Member(self, h, 3, 2, True, False)
        m._keepalive = [a, b]
        return m

    def member_split_eq_uniform(self, tables, V, F, coeffs, w, scale=None, shard_scale=None, borrow=False):
        """eq(w,.) * sum_v coeffs[v] * prod_{i<F} tables[v*F+i]; prove_round returns q(0), q(2), .., q(F)."""
        w = fr(w).reshape(-1, 4)
        co = np.ascontiguousarray(np.stack([fr(c) for c in coeffs])).reshape(-1, 4)
        hs = (C.c_void_p * len(tables))(*[t.h for t in tables])
        h = C.c_void_p()
        _call("jolt_member_create_split_eq_uniform", self, self.h, hs, V, F, _p(co), _p(w), w.shape[0], _p(fr(scale)) if scale is not None else None,
              _p(fr(shard_scale)) if shard_scale is not None else None, MEMBER_FLAG_BORROW_TABLES if borrow else 0, C.byref(h))
        m = Member(self, h, F + 1, len(tables), True, False)
        m.n_evals = F
        m.uniform = True
        if borrow:
            m._keepalive = list(tables)
        else:
            for t in tables:
                t.h = None
        return m

    def round_group_prove(self, members, binds):
        hs = (C.c_void_p * len(members))(*[m.h for m in members])
        bstore = [None if b is None else fr(b) for b in binds]
        bp = (C.c_void_p * len(members))(*[None if b is None else b.ctypes.data for b in bstore])
        total = sum(m.n_evals for m in members)
        out = fr_array(total)
        _call("jolt_round_group_prove", self, self.h, hs, len(members), bp, _p(out), total)
        res, off = [], 0
        for m in members:
            res.append(out[off:off + m.n_evals].copy())
            off += m.n_evals
        return res

    def prove_batch(self, members, input_claims, coefficients, offsets, max_num_vars, max_degree, label=0, challenge_mode=0,
                    use_round_group=True):
        n = len(members)
        hs = (C.c_void_p * n)(*[m.h for m in members])
        ic = np.ascontiguousarray(np.stack(input_claims), dtype=np.uint64).reshape(-1, 4)
        co = np.ascontiguousarray(np.stack(coefficients), dtype=np.uint64).reshape(-1, 4)
        offs = (C.c_size_t * n)(*offsets)
        polys, chal = fr_array(max_num_vars * (max_degree + 1)), fr_array(max_num_vars)
        mclaims, final = fr_array(n), fr_array(1)
        _call("jolt_host_prove_batch", self, self.h, hs, n, _p(ic), _p(co), offs, max_num_vars, max_degree, label, challenge_mode, 1 if use_round_group else 0, _p(polys),
              _p(chal), _p(mclaims), _p(final))
        return dict(polys=polys.reshape(max_num_vars, max_degree + 1, 4), challenges=chal, member_claims=mclaims, final_claim=final[0])

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Table:
    def __init__(self, ctx, handle):
        self.ctx, self.h = ctx, handle

    def __len__(self):
        n = C.c_size_t()
        _call("jolt_table_len", self.ctx, self.h, C.byref(n))
        return n.value

    def download(self, offset=0, length=None):
        n = len(self) - offset if length is None else length
        out = fr_array(n)
        _call("jolt_table_download", self.ctx, self.ctx.h, self.h, offset, n, _p(out))
        return out

    def clone(self):
        h = C.c_void_p()
        _call("jolt_table_clone", self.ctx, self.ctx.h, self.h, C.byref(h))
        return Table(self.ctx, h)

    def device_ptr(self):
        p = C.c_void_p()
        _call("jolt_table_device_ptr", self.ctx, self.h, C.byref(p))
        return p.value

    def free(self):
        if self.h and self.ctx.h:
            lib().jolt_table_free(self.ctx.h, self.h)
        self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Member:
    """Handle of a device-resident sumcheck member (jolt_sumcheck::ProveRounds, device half)."""

    def __init__(self, ctx, handle, degree, n_tables, split_eq, skip_one):
        self.ctx, self.h, self.degree, self.n_tables, self.split_eq, self.skip_one = ctx, handle, degree, n_tables, split_eq, skip_one
        self.n_evals = 2 if split_eq else (degree if skip_one else degree + 1)
        self.uniform = False

    def set_scale(self, scale):
        _call("jolt_member_set_scale", self.ctx, self.h, _p(fr(scale)))

    def num_rounds(self):
        n = C.c_size_t()
        _call("jolt_member_num_rounds", self.ctx, self.h, C.byref(n))
        return n.value

    def prove_round(self, bind=None, want_aux=False):
        out, aux = fr_array(self.n_evals), fr_array(3)
        _call("jolt_member_prove_round", self.ctx, self.h, _p(fr(bind)) if bind is not None else None, _p(out), self.n_evals, _p(aux))
        return (out, aux) if want_aux else out

    def finish(self, bind):
        _call("jolt_member_finish", self.ctx, self.h, _p(fr(bind)))

    def final_values(self):
        k = self.n_tables + (1 if self.split_eq else 0)
        out = fr_array(k)
        _call("jolt_member_final_values", self.ctx, self.h, _p(out), k)
        return out

    def input_claim(self):
        out = fr_array(1)
        _call("jolt_member_input_claim", self.ctx, self.h, _p(out))
        return out[0]

    def reset(self):
        _call("jolt_member_reset", self.ctx, self.h)

    def destroy(self):
        if self.h and self.ctx.h:
            lib().jolt_member_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


# ---- host-side helpers (no GPU needed) ------------------------------------------------------------------------------
def host_fr_binop(name, a, b):
    o = fr_array(1)
    _call(name, None, _p(fr(a)), _p(fr(b)), _p(o))
    return o[0]


def host_fr_mul(a, b): return host_fr_binop("jolt_host_fr_mul", a, b)


def host_mul_limbs29(field, a, b):
    """the device multiplication algorithm (29-bit limbs) built for the host; field 0 = Fr, 1 = Fq"""
    o = fr_array(1)
    _call("jolt_host_mul_limbs29", None, field, _p(fr(a)), _p(fr(b)), _p(o))
    return o[0]


def host_fr_wide_dot(a, b):
    """sum_k a[k]*b[k] through the deferred-reduction accumulator (one REDC per block of products)"""
    a = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 4)
    b = np.ascontiguousarray(b, dtype=np.uint64).reshape(-1, 4)
    o = fr_array(1)
    _call("jolt_host_fr_wide_dot", None, _p(a), _p(b), a.shape[0], _p(o))
    return o[0]

def host_fr_add(a, b): return host_fr_binop("jolt_host_fr_add", a, b)
def host_fr_sub(a, b): return host_fr_binop("jolt_host_fr_sub", a, b)
def host_fr_mul_shifted(a, c): return host_fr_binop("jolt_host_fr_mul_shifted", a, c)


def host_fr_inv(a):
    o = fr_array(1)
    _call("jolt_host_fr_inv", None, _p(fr(a)), _p(o))
    return o[0]


def host_fr_from_u64(v):
    o = fr_array(1)
    _call("jolt_host_fr_from_u64", None, v, _p(o))
    return o[0]


def host_eq_evals(r, scale=None):
    p = fr(r).reshape(-1, 4)
    out = fr_array(1 << p.shape[0])
    st = lib().jolt_host_eq_evals(_p(p), p.shape[0], _p(fr(scale)) if scale is not None else None, _p(out))
    if st != 0:
        raise JoltError(st, "jolt_host_eq_evals")
    return out


def host_univariate_from_evals(evals):
    e = fr(evals).reshape(-1, 4)
    o = fr_array(e.shape[0])
    _call("jolt_host_univariate_from_evals", None, _p(e), e.shape[0], _p(o))
    return o


def host_univariate_evaluate(coeffs, x):
    c = fr(coeffs).reshape(-1, 4)
    o = fr_array(1)
    _call("jolt_host_univariate_evaluate", None, _p(c), c.shape[0], _p(fr(x)), _p(o))
    return o[0]


def host_gruen_poly_from_q(scalar, point_i, q_evals, claim):
    q = fr(q_evals).reshape(-1, 4)
    o = fr_array(q.shape[0] + 2)
    _call("jolt_host_gruen_poly_from_q", None, _p(fr(scalar)), _p(fr(point_i)), _p(q), q.shape[0], _p(fr(claim)), _p(o))
    return o


class HostBooleanityAddress:
    """The K-domain state of the booleanity address phase on the host (jolt_host_booleanity_address_*): masses (n_polys, K, 4) from the pushforward"""

    def __init__(self, masses, gamma, reference_address):
        self.linear = np.ascontiguousarray(masses, dtype=np.uint64).copy()
        self.squared = self.linear.copy()
        self.n_polys, self.k = self.linear.shape[0], self.linear.shape[1]
        self.len = self.k
        g2 = host_fr_mul(gamma, gamma)
        w, cur = [], host_fr_from_u64(1)
        for _ in range(self.n_polys):
            w.append(cur)
            cur = host_fr_mul(cur, g2)
        self.weights = np.ascontiguousarray(np.stack(w))
        self.eq = np.ascontiguousarray(host_eq_evals(reference_address)).copy()

    def round(self):
        o = fr_array(4)
        _call("jolt_host_booleanity_address_round", None, _p(self.linear), _p(self.squared), self.n_polys, self.k, self.len, _p(self.weights), _p(self.eq), _p(o))
        return o

    def bind(self, r):
        _call("jolt_host_booleanity_address_bind", None, _p(self.linear), _p(self.squared), self.n_polys, self.k, self.len, _p(self.eq), _p(fr(r)))
        self.len //= 2

    def intermediate(self):
        assert self.len == 1
        acc = np.zeros(4, dtype=np.uint64)
        for i in range(self.n_polys):
            acc = host_fr_add(acc, host_fr_mul(self.weights[i], host_fr_sub(self.squared[i, 0], self.linear[i, 0])))
        return host_fr_mul(self.eq[0], acc)


class HostHammingWeight:
    """HammingWeightKernel's K_chunk-domain state on the host (jolt_host_hamming_weights / jolt_host_pair_tables_*): masses (n_polys, K, 4) from the pushforward"""

    def __init__(self, masses, gamma, r_address, virtualization_points):
        self.g = np.ascontiguousarray(masses, dtype=np.uint64).copy()
        self.n_polys, self.k = self.g.shape[0], self.g.shape[1]
        self.len = self.k
        log_k = self.k.bit_length() - 1
        ra = np.ascontiguousarray(fr(r_address), dtype=np.uint64).reshape(-1, 4)
        vp = np.ascontiguousarray(virtualization_points, dtype=np.uint64).reshape(-1, 4)
        assert ra.shape[0] == log_k and vp.shape[0] == self.n_polys * log_k
        self.w = fr_array(self.n_polys * self.k).reshape(self.n_polys, self.k, 4)
        _call("jolt_host_hamming_weights", None, _p(fr(gamma)), _p(ra), _p(vp), self.n_polys, log_k, _p(self.w))

    def round(self):
        o = fr_array(3)
        _call("jolt_host_pair_tables_round", None, _p(self.g), _p(self.w), self.n_polys, self.k, self.len, _p(o))
        return o

    def bind(self, r):
        _call("jolt_host_pair_tables_bind", None, _p(self.g), _p(self.w), self.n_polys, self.k, self.len, _p(fr(r)))
        self.len //= 2

    def output_claims(self):
        assert self.len == 1
        return self.g[:, 0].copy()


TRANSCRIPT_TEST, TRANSCRIPT_BLAKE2B, TRANSCRIPT_KECCAK, TRANSCRIPT_BLAKE2B_SPONGE = (abi.CONSTANTS["JOLT_TRANSCRIPT_" + k] << 62 for k in ("TEST", "BLAKE2B_LEGACY", "KECCAK_SPONGE", "BLAKE2B_SPONGE"))  # OR into any `label` / `transcript_label`: the engine behind it (include/jolt_hip.h)


class HostTranscript:
    """jolt_host_transcript_*: the library's transcripts for members driven round by round from here.  `label`: an integer whose two top bits select the engine
    (TRANSCRIPT_TEST: the deterministic test transcript; TRANSCRIPT_BLAKE2B: the reference's LegacyBlake2bTranscript, the one its benchmark profile proves with;
    TRANSCRIPT_KECCAK: its KeccakTranscript), or a byte label with `kind` 1 / 2 -- the reference's `Transcript::new(b"...")`."""

    def __init__(self, label, kind=None):
        self.h = C.c_void_p()
        if isinstance(label, (bytes, bytearray)):
            buf = (C.c_uint8 * max(1, len(label))).from_buffer_copy(bytes(label) if len(label) else b"\0")
            _call("jolt_host_transcript_create_labelled", None, kind, buf, len(label), C.byref(self.h))
        else:
            _call("jolt_host_transcript_create", None, label, C.byref(self.h))

    def append(self, values):
        v = np.ascontiguousarray(values, dtype=np.uint64).reshape(-1, 4)
        _call("jolt_host_transcript_append_fr", None, self.h, _p(v), v.shape[0])

    def append_bytes(self, data):
        buf = (C.c_uint8 * max(1, len(data))).from_buffer_copy(bytes(data) if len(data) else b"\0")
        _call("jolt_host_transcript_append_bytes", None, self.h, buf, len(data))

    def append_label(self, label, count=None):
        _call("jolt_host_transcript_append_label", None, self.h, C.c_char_p(label), 0 if count is None else 1, count or 0)

    def append_u64_word(self, value):
        _call("jolt_host_transcript_append_u64_word", None, self.h, value)

    def append_round_poly(self, coefficients, label=b"sumcheck_poly"):
        v = np.ascontiguousarray(coefficients, dtype=np.uint64).reshape(-1, 4)
        _call("jolt_host_transcript_append_round_poly", None, self.h, C.c_char_p(label), _p(v), v.shape[0])

    def state(self):
        out = (C.c_uint8 * 32)()
        _call("jolt_host_transcript_state", None, self.h, out)
        return bytes(out)

    def challenge(self, full_width=False):
        o = fr_array(1)
        _call("jolt_host_transcript_challenge", None, self.h, 1 if full_width else 0, _p(o))
        return o[0]

    def clone(self):
        """an independent copy in the current state (jolt_host_transcript_clone)"""
        c = HostTranscript.__new__(HostTranscript)
        c.h = C.c_void_p()
        _call("jolt_host_transcript_clone", None, self.h, C.byref(c.h))
        return c

    def close(self):
        if self.h:
            lib().jolt_host_transcript_destroy(self.h)
            self.h = None


def host_blake2b(data, outlen=32):
    out = (C.c_uint8 * outlen)()
    buf = (C.c_uint8 * max(1, len(data))).from_buffer_copy(bytes(data) if len(data) else b"\0")
    _call("jolt_host_blake2b", None, buf, len(data), outlen, out)
    return bytes(out)


def host_keccak_f1600(state):
    buf = (C.c_uint8 * 200).from_buffer_copy(bytes(state))
    _call("jolt_host_keccak_f1600", None, buf)
    return bytes(buf)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def host_gruen_poly_deg_3(scalar, point_i, q0, qinf, claim):
    o = fr_array(4)
    _call("jolt_host_gruen_poly_deg_3", None, _p(fr(scalar)), _p(fr(point_i)), _p(fr(q0)), _p(fr(qinf)), _p(fr(claim)), _p(o))
    return o


# ---- G1 / MSM / HyperKZG ---------------------------------------------------------------------------------------------
class Srs:
    """Device-resident affine bases (HyperKZGProverSetup.g1_powers)."""

    def __init__(self, ctx, handle):
        self.ctx, self.h = ctx, handle

    def __len__(self):
        n = C.c_size_t()
        _call("jolt_srs_len", self.ctx, self.h, C.byref(n))
        return n.value

    def download(self, offset=0, n=None):
        n = len(self) - offset if n is None else n
        out = g1_array(n)
        _call("jolt_srs_download", self.ctx, self.ctx.h, self.h, offset, n, _p(out))
        return out

    def free(self):
        if self.h and self.ctx.h:
            lib().jolt_srs_free(self.ctx.h, self.h)
        self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _srs_upload(self, bases):
    b = np.ascontiguousarray(bases, dtype=np.uint64).reshape(-1, 12)
    h = C.c_void_p()
    _call("jolt_srs_upload_g1", self, self.h, _p(b), b.shape[0], C.byref(h))
    return Srs(self, h)


def _srs_setup_from_secret(self, beta, count, g1):
    h = C.c_void_p()
    _call("jolt_srs_setup_from_secret", self, self.h, _p(fr(beta)), count, _p(np.ascontiguousarray(g1, dtype=np.uint64)), C.byref(h))
    return Srs(self, h)


def host_owned_terms(n, block, rank, world):
    """Terms of the prefix [0, n) that `rank` owns under the block-cyclic assignment (host only)."""
    out = C.c_size_t()
    _call("jolt_host_owned_terms", None, n, block, rank, world, C.byref(out))
    return out.value


def host_subtree_owned_terms(n, rank, world):
    """Terms of the prefix [0, n) that `rank` owns under the subtree assignment (host only)."""
    out = C.c_size_t()
    _call("jolt_host_subtree_owned_terms", None, n, rank, world, C.byref(out))
    return out.value


def host_subtree_term_index(slot, rank, world):
    """Index of the rank's compact slot under the subtree assignment (host only)."""
    out = C.c_size_t()
    _call("jolt_host_subtree_term_index", None, slot, rank, world, C.byref(out))
    return out.value


def _srs_setup_from_secret_subtree(self, beta, count_global, g1, rank, world):
    """One rank's compact share of the powers under the subtree assignment."""
    h = C.c_void_p()
    _call("jolt_srs_setup_from_secret_subtree", self, self.h, _p(fr(beta)), count_global, _p(np.ascontiguousarray(g1, dtype=np.uint64)), rank, world, C.byref(h))
    return Srs(self, h)


def _msm_subtree(self, srs, table, n, rank, world):
    """The rank's share of sum_{i<n} table[i] * SRS[i] under the subtree assignment (srs = the rank's compact SRS)."""
    out = g1_array(1)
    _call("jolt_msm_g1_table_subtree", self, self.h, srs.h, table.h, n, rank, world, _p(out))
    return out[0]


def _hyperkzg_open_subtree(self, srs, evals_compact, point, label, rank, world, gather_fn, gather_user):
    """jolt_host_hyperkzg_open_subtree: the opening with the polynomial sharded over the ranks (evals_compact: the rank's compact array)."""
    p = fr(point).reshape(-1, 4)
    ell = p.shape[0]
    com, w, v, ch = g1_array(max(ell - 1, 1)), g1_array(3), fr_array(3 * ell), fr_array(3)
    _call("jolt_host_hyperkzg_open_subtree", self, self.h, srs.h, evals_compact.h, _p(p), ell, label, rank, world, gather_fn, gather_user, _p(com), _p(w), _p(v), _p(ch))
    return dict(com=com[: ell - 1], w=w, v=v.reshape(3, ell, 4), challenges=ch)


def _srs_setup_from_secret_blocks(self, beta, count_global, g1, block, rank, world):
    """One rank's compact share of the powers under the block-cyclic term assignment (term i belongs to rank (i / block) % world)."""
    h = C.c_void_p()
    _call("jolt_srs_setup_from_secret_blocks", self, self.h, _p(fr(beta)), count_global, _p(np.ascontiguousarray(g1, dtype=np.uint64)), block, rank, world, C.byref(h))
    return Srs(self, h)


def _msm_blocks(self, srs, table, n, block, rank, world):
    """The rank's share of sum_{i<n} table[i] * SRS[i] under the block-cyclic assignment (srs = the rank's compact SRS)."""
    out = g1_array(1)
    _call("jolt_msm_g1_table_blocks", self, self.h, srs.h, table.h, n, block, rank, world, _p(out))
    return out[0]


class PendingMsms:
    """jolt_msm_g1_tables_begin ... _finish: up to three prefix MSMs in flight on the side lanes while the caller works on the main stream"""

    def __init__(self, ctx, srs, tables, ns):
        hs = (C.c_void_p * len(tables))(*[t.h for t in tables])
        nn = (C.c_size_t * len(tables))(*[int(x) for x in ns])
        h = C.c_void_p()
        _call("jolt_msm_g1_tables_begin", ctx, ctx.h, srs.h, hs, nn, len(tables), C.byref(h))
        self.ctx, self.h, self.count = ctx, h, len(tables)

    def finish(self):
        out = g1_array(self.count)
        h, self.h = self.h, None
        _call("jolt_msm_g1_tables_finish", self.ctx, self.ctx.h, h, _p(out))
        return out


def _msm_tables_begin(self, srs, tables, ns):
    return PendingMsms(self, srs, tables, ns)


def _msm(self, srs, scalars, n=None, full_width=False):
    """JoltGroup::msm(bases = srs[..n], scalars); scalars = numpy (n,4) host array or a device Table.  full_width: the caller knows the scalars to be uniform field
    elements (jolt_msm_g1_table_full_width)."""
    out = g1_array(1)
    if isinstance(scalars, Table):
        n = len(scalars) if n is None else n
        fn = "jolt_msm_g1_table_full_width" if full_width else "jolt_msm_g1_table"
        _call(fn, self, self.h, srs.h, scalars.h, n, _p(out))
    else:
        s = fr(scalars).reshape(-1, 4)
        n = s.shape[0] if n is None else n
        _call("jolt_msm_g1", self, self.h, srs.h, _p(s), n, _p(out))
    return out[0]


def _msm_profile_buckets(self, enable=True):
    """HIP events around the bucket-sum kernel of every later fixed-base MSM (jolt_msm_profile_buckets)"""
    _call("jolt_msm_profile_buckets", self, self.h, 1 if enable else 0)


def _msm_profile_buckets_last(self):
    """(milliseconds, mixed additions) of the last profiled bucket-sum launch"""
    ms, adds = C.c_float(), C.c_uint64()
    _call("jolt_msm_profile_buckets_last", self, self.h, C.byref(ms), C.byref(adds))
    return float(ms.value), int(adds.value)


FX_PLAN_FIELDS = ("c", "W", "lo_bits", "soa", "wide", "capacity", "two_pass", "grid_reduce", "heavy_threshold", "stage_cap", "nb1", "max_lds_per_block",
                  "overflow", "largest_segment", "heavy_segments")


def _msm_fixed_last_plan(self):
    """The plan of the context's last fixed-base MSM (jolt_msm_fixed_last_plan) as a dict over FX_PLAN_FIELDS: the host's decisions (flags as bools), then the three
    words the sort left on the device -- None once a later job has reused the workspace they live in.  Raises JoltError (invalid argument) before the first
    fixed-base MSM of the context."""
    a = np.zeros(FX_PLAN_WORDS, dtype=np.uint32)
    _call("jolt_msm_fixed_last_plan", self, self.h, _p(a), FX_PLAN_WORDS)
    out = {name: int(a[k]) for k, name in enumerate(FX_PLAN_FIELDS)}
    for name in ("soa", "wide", "capacity", "two_pass", "grid_reduce"):
        out[name] = bool(out[name])
    for name in ("overflow", "largest_segment", "heavy_segments"):
        if out[name] == FX_PLAN_STALE:
            out[name] = None
    return out


def _measure_mad_peak(self, target_ms=50.0):
    """jolt_ctx_measure_mad_peak: (v_mad_u64_u32 lane-operations per second chip-wide, kernel milliseconds timed, launches)"""
    rate, ms, n = C.c_double(), C.c_float(), C.c_uint32()
    _call("jolt_ctx_measure_mad_peak", self, self.h, target_ms, C.byref(rate), C.byref(ms), C.byref(n))
    return float(rate.value), float(ms.value), int(n.value)


def _msm_window(self, srs, base_offset, values, kind=None, acc=None):
    """One window of a streamed commitment (jolt_msm_g1_window: StreamingCommitment::feed / feed_u64 / feed_i128 for a KZG-type scheme): acc + sum_i values[i] *
    srs[base_offset + i].  values: (n, 4) uint64 field elements (kind "fr"), uint64 / int64 arrays, or i128 as an (n, 2) uint64 array (kind "i128")."""
    v = np.ascontiguousarray(values)
    if kind is None:
        kind = "fr" if (v.ndim == 2 and v.shape[1] == 4) else ({np.dtype(np.uint64): "u64", np.dtype(np.int64): "i64"}[v.dtype] if v.ndim == 1 else "i128")
    code = {"u64": 0, "i64": 1, "i128": 2, "fr": 3}[kind]
    out = g1_array(1)
    a = None if acc is None else np.ascontiguousarray(acc, dtype=np.uint64).reshape(-1)
    _call("jolt_msm_g1_window", self, self.h, srs.h, base_offset, code, v.ctypes.data_as(C.c_void_p), v.shape[0], None if a is None else _p(a), _p(out))
    return out[0]


def _hyperkzg_fold(self, evals, point):
    p = fr(point).reshape(-1, 4)
    ell = p.shape[0]
    hs = (C.c_void_p * max(ell, 1))()
    _call("jolt_hyperkzg_fold", self, self.h, evals.h, _p(p), ell, hs)
    return [Table(self, C.c_void_p(hs[i])) for i in range(ell)]


def _hyperkzg_eval3(self, levels, u):
    hs = (C.c_void_p * len(levels))(*[t.h for t in levels])
    uu = fr(u).reshape(3, 4)
    out = fr_array(3 * len(levels))
    _call("jolt_hyperkzg_eval3", self, self.h, hs, len(levels), _p(uu), _p(out))
    return out.reshape(3, len(levels), 4)


def _hyperkzg_rlc(self, levels, q):
    hs = (C.c_void_p * len(levels))(*[t.h for t in levels])
    h = C.c_void_p()
    _call("jolt_hyperkzg_rlc", self, self.h, hs, len(levels), _p(fr(q)), C.byref(h))
    return Table(self, h)


def _hyperkzg_witness_poly(self, f, u):
    h = C.c_void_p()
    _call("jolt_hyperkzg_witness_poly", self, self.h, f.h, _p(fr(u)), C.byref(h))
    return Table(self, h)


def _hyperkzg_commit(self, srs, evals):
    out = g1_array(1)
    _call("jolt_host_hyperkzg_commit", self, self.h, srs.h, evals.h, _p(out))
    return out[0]


def _hyperkzg_open(self, srs, evals, point, label=0, known_levels=None):
    """known_levels: (n, 12) commitments of the first n folded polynomials, computed by the caller (jolt_host_hyperkzg_open_with_levels skips their MSMs)"""
    p = fr(point).reshape(-1, 4)
    ell = p.shape[0]
    com, w, v, ch = g1_array(max(ell - 1, 1)), g1_array(3), fr_array(3 * max(ell, 1)), fr_array(3)
    if known_levels is not None and len(known_levels):
        kl = np.ascontiguousarray(known_levels, dtype=np.uint64).reshape(-1, 12)
        _call("jolt_host_hyperkzg_open_with_levels", self, self.h, srs.h, evals.h, _p(p), ell, label, None, None, _p(kl), kl.shape[0], _p(com), _p(w), _p(v), _p(ch))
        return dict(com=com[: ell - 1], w=w, v=v.reshape(3, ell, 4), challenges=ch)
    _call("jolt_host_hyperkzg_open", self, self.h, srs.h, evals.h, _p(p), ell, label, _p(com), _p(w), _p(v), _p(ch))
    return dict(com=com[: ell - 1], w=w, v=v.reshape(3, ell, 4), challenges=ch)


class GridHint:
    """The commitment grid's opening hint (jolt_grid_hint_begin): the class sums of the one-hot columns for the first `levels` level commitments of an opening, in
    flight on the context's background stream (or its main stream) from the moment this returns"""

    def __init__(self, ctx, srs, sources, levels, background=True):
        hs = (C.c_void_p * len(sources))(*[s_.h for s_ in sources])
        h = C.c_void_p()
        _call("jolt_grid_hint_begin", ctx, ctx.h, srs.h, hs, len(sources), levels, 1 if background else 0, C.byref(h))
        self.ctx, self.h, self.levels, self.n_cols, self._keep = ctx, h, levels, sum(s_.n_polys for s_ in sources), list(sources)

    def wait(self):
        _call("jolt_grid_hint_wait", self.ctx, self.ctx.h, self.h)

    def download(self, level):
        out = g1_array(self.n_cols << level)
        _call("jolt_grid_hint_download", self.ctx, self.ctx.h, self.h, level, _p(out))
        return out.reshape(1 << level, self.n_cols, 12)

    def free(self):
        if self.h:
            lib().jolt_grid_hint_free(self.ctx.h, self.h)
            self.h = None
        self._keep = []

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _hyperkzg_open_grid(self, srs, evals, point, hint, levels, onehot_scalars, dense, dense_scalars, label=0, callback=None):
    """jolt_host_hyperkzg_open_grid: the opening of the grid's joint polynomial with its first `levels` level commitments by linearity from the commit-time hint.
    callback (phase, points (n, 12), values (n, 4)) -> challenge (4,): the caller's transcript in place of the library's under `label`"""
    p = fr(point).reshape(-1, 4)
    ell = p.shape[0]
    com, w, v, ch = g1_array(max(ell - 1, 1)), g1_array(3), fr_array(3 * max(ell, 1)), fr_array(3)
    osc = np.ascontiguousarray(onehot_scalars, dtype=np.uint64).reshape(-1, 4)
    dsc = np.ascontiguousarray(dense_scalars, dtype=np.uint64).reshape(-1, 4) if len(dense) else None
    hs = (C.c_void_p * max(len(dense), 1))(*[t.h for t in dense])
    fn, err = open_transcript_callback(callback) if callback is not None else (None, [])
    st = lib().jolt_host_hyperkzg_open_grid(self.h, srs.h, evals.h, _p(p), ell, label, fn, None, hint.h, levels, _p(osc), hs, len(dense),
                                            _p(dsc) if dsc is not None else None, _p(com), _p(w), _p(v), _p(ch))
    if err:
        raise err[0]
    _ck(st, "jolt_host_hyperkzg_open_grid", self)
    return dict(com=com[: ell - 1], w=w, v=v.reshape(3, ell, 4), challenges=ch)


def _srs_precompute_windows(self, srs, window_bits=0, min_terms=0):
    """Fixed-base tables 2^(c*w) * srs[i] (one bucket set for all windows of an MSM): ceil(255/c) copies of the bases in HBM."""
    _call("jolt_srs_precompute_windows", self, self.h, srs.h, window_bits, min_terms)


def _srs_precompute_grid_pairs(self, srs, k, cycles, shifts=(0,)):
    """Pair tables of the k x cycles commitment grid for the given shifts (jolt_srs_precompute_grid_pairs): the one-hot sums of bases over an SRS with window
    tables then add one entry per pair of cycles.  A table that cannot be built is left out; returns the bytes the SRS holds for (k, cycles >> s), per shift."""
    _call("jolt_srs_precompute_grid_pairs", self, self.h, srs.h, k, cycles, sum(1 << s for s in set(shifts)))
    return {s: srs_grid_pairs_bytes(srs, k, cycles >> s) for s in sorted(set(shifts))}


def srs_grid_pairs_bytes(srs, k, domain):
    out = C.c_size_t()
    _call("jolt_srs_grid_pairs_bytes", srs.ctx, srs.h, k, domain, C.byref(out))
    return out.value


def host_grid_pair_entry(p, q):
    """(8,) words of the pair-table entry for p + q (L-form affine x, y; zeros = infinity), from the host twin of the builder's arithmetic"""
    out = np.zeros(8, dtype=np.uint64)
    _call("jolt_host_grid_pair_entry", None, _p(np.ascontiguousarray(p, dtype=np.uint64)), _p(np.ascontiguousarray(q, dtype=np.uint64)), _p(out))
    return out


def host_grid_pair_index(m, k, a, b):
    out = C.c_size_t()
    _call("jolt_host_grid_pair_index", None, m, k, a, b, C.byref(out))
    return out.value


Context.srs_precompute_windows = _srs_precompute_windows
Context.srs_precompute_grid_pairs = _srs_precompute_grid_pairs
Context.srs_upload = _srs_upload
Context.srs_setup_from_secret = _srs_setup_from_secret
Context.msm = _msm
Context.msm_window = _msm_window
Context.msm_profile_buckets = _msm_profile_buckets
Context.msm_profile_buckets_last = _msm_profile_buckets_last
Context.msm_fixed_last_plan = _msm_fixed_last_plan
Context.measure_mad_peak = _measure_mad_peak
Context.srs_setup_from_secret_blocks = _srs_setup_from_secret_blocks
Context.msm_blocks = _msm_blocks
Context.srs_setup_from_secret_subtree = _srs_setup_from_secret_subtree
Context.msm_subtree = _msm_subtree
Context.hyperkzg_open_subtree = _hyperkzg_open_subtree
Context.hyperkzg_fold = _hyperkzg_fold
Context.msm_tables_begin = _msm_tables_begin
Context.hyperkzg_eval3 = _hyperkzg_eval3
Context.hyperkzg_rlc = _hyperkzg_rlc
Context.hyperkzg_witness_poly = _hyperkzg_witness_poly
Context.hyperkzg_commit = _hyperkzg_commit
Context.hyperkzg_open = _hyperkzg_open
Context.hyperkzg_open_grid = _hyperkzg_open_grid
Context.grid_hint = lambda self, srs, sources, levels, background=True: GridHint(self, srs, sources, levels, background)

OPEN_TRANSCRIPT_FN = abi.CALLBACK_TYPES["jolt_open_transcript_fn"]


def open_transcript_callback(callback):
    """a jolt_open_transcript_fn around callback(phase, points (n, 12), values (n, 4)) -> challenge (4,) or a non-zero status; -> (fn, err): an exception of the
    callback never unwinds through the C frame, it ends the call with status 4 and waits in err"""
    err = []

    def cb(user, phase, points, n_points, values, n_values, out):
        try:
            take = lambda p, k, wd: np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint64)), shape=(k, wd)).copy() if k else np.zeros((0, wd), dtype=np.uint64)  # noqa: E731
            c = callback(phase, take(points, n_points, 12), take(values, n_values, 4))
            if isinstance(c, (int, np.integer)) and not isinstance(c, bool):
                return int(c)
            c = np.ascontiguousarray(c, dtype=np.uint64).reshape(4)
            C.memmove(out, c.ctypes.data, 32)
            return 0
        except Exception as e:
            err.append(e)
            return 4

    return OPEN_TRANSCRIPT_FN(cb), err


def _hyperkzg_open_with_transcript(self, srs, evals, point, absorb_points, absorb_values, challenge):
    """jolt_host_hyperkzg_open_with_transcript: the opening under the CALLER's transcript.  absorb_points((n, 12) Jacobian limbs) / absorb_values((n, 4)) absorb what
    the prover sends at a step, challenge() -> (4,) draws the challenge after it (three steps: level commitments -> r, evaluations -> q, witness commitments -> d_0)."""
    p = fr(point).reshape(-1, 4)
    ell = p.shape[0]
    com, w, v, ch = g1_array(max(ell - 1, 1)), g1_array(3), fr_array(3 * max(ell, 1)), fr_array(3)
    err = []

    def cb(user, phase, points, n_points, values, n_values, out):
        try:
            if n_points:
                absorb_points(np.ctypeslib.as_array(C.cast(points, C.POINTER(C.c_uint64)), shape=(n_points, 12)).copy())
            if n_values:
                absorb_values(np.ctypeslib.as_array(C.cast(values, C.POINTER(C.c_uint64)), shape=(n_values, 4)).copy())
            c = np.ascontiguousarray(challenge(), dtype=np.uint64).reshape(4)
            C.memmove(out, c.ctypes.data, 32)
            return 0
        except Exception as e:  # never unwind through the C frame
            err.append(e)
            return 4

    fn = OPEN_TRANSCRIPT_FN(cb)
    st = lib().jolt_host_hyperkzg_open_with_transcript(self.h, srs.h, evals.h, _p(p), ell, fn, None, _p(com), _p(w), _p(v), _p(ch))
    if err:
        raise err[0]
    _ck(st, "jolt_host_hyperkzg_open_with_transcript", self)
    return dict(com=com[: ell - 1], w=w, v=v.reshape(3, ell, 4), challenges=ch)


Context.hyperkzg_open_with_transcript = _hyperkzg_open_with_transcript


def host_g1_add(p, q):
    o = g1_array(1)
    _call("jolt_host_g1_add", None, _p(np.ascontiguousarray(p, dtype=np.uint64)), _p(np.ascontiguousarray(q, dtype=np.uint64)), _p(o))
    return o[0]


def host_g1_is_on_curve(p):
    e = C.c_int32()
    _call("jolt_host_g1_is_on_curve", None, _p(np.ascontiguousarray(p, dtype=np.uint64)), C.byref(e))
    return bool(e.value)


def host_g1_eq(p, q):
    e = C.c_int32()
    _call("jolt_host_g1_eq", None, _p(np.ascontiguousarray(p, dtype=np.uint64)), _p(np.ascontiguousarray(q, dtype=np.uint64)), C.byref(e))
    return bool(e.value)


def host_g1_serialize_compressed(p):
    out = (C.c_uint8 * 32)()
    _call("jolt_host_g1_serialize_compressed", None, _p(np.ascontiguousarray(p, dtype=np.uint64)), out)
    return bytes(out)


class PinnedBuffer:
    """Page-locked host memory (jolt_host_pinned_alloc) as a numpy uint8 array of the given shape: the staging block a tracer fills and Rows uploads from"""

    def __init__(self, ctx, shape):
        shape = tuple(int(x) for x in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        n = int(np.prod(shape))
        p = C.c_void_p()
        _call("jolt_host_pinned_alloc", ctx, ctx.h, n, C.byref(p))
        self.ctx, self.p = ctx, p
        self.array = np.ctypeslib.as_array((C.c_uint8 * n).from_address(p.value)).reshape(shape)

    def free(self):
        if self.p:
            self.array = None
            _call("jolt_host_pinned_free", self.ctx, self.ctx.h, self.p)
            self.p = None


class Rows:
    """Packed typed witness rows (numpy structured or 2-D uint8 array) resident on the device; columns are expanded there."""

    def __init__(self, ctx, rows):
        raw = np.ascontiguousarray(rows)
        self.n_rows, self.row_bytes = raw.shape[0], raw.dtype.itemsize if raw.ndim == 1 else raw.shape[1]
        h = C.c_void_p()
        _call("jolt_rows_upload", ctx, ctx.h, raw.ctypes.data_as(C.c_void_p), self.n_rows, self.row_bytes, C.byref(h))
        self.ctx, self.h = ctx, h

    @classmethod
    def begin(cls, ctx, pinned_rows):
        """jolt_rows_upload_begin: the copy starts now on the context's copy stream and runs beside whatever the context does next; `pinned_rows` is a PinnedBuffer's
        array (page-locked) and must stay unchanged until wait()"""
        raw = pinned_rows
        assert raw.flags["C_CONTIGUOUS"] and raw.ndim == 2
        self = cls.__new__(cls)
        self.n_rows, self.row_bytes = raw.shape[0], raw.shape[1]
        h = C.c_void_p()
        _call("jolt_rows_upload_begin", ctx, ctx.h, raw.ctypes.data_as(C.c_void_p), self.n_rows, self.row_bytes, C.byref(h))
        self.ctx, self.h = ctx, h
        return self

    def wait(self):
        _call("jolt_rows_upload_wait", self.ctx, self.ctx.h, self.h)

    def table(self, offset, width, signed=False):
        h = C.c_void_p()
        _call("jolt_table_from_rows", self.ctx, self.ctx.h, self.h, offset, width, 1 if signed else 0, C.byref(h))
        return Table(self.ctx, h)

    def ints(self, offset, width, signed=False):
        """the field as a resident integer column (jolt_ints_from_rows): compact scalars, no promotion"""
        h = C.c_void_p()
        _call("jolt_ints_from_rows", self.ctx, self.ctx.h, self.h, offset, width, 1 if signed else 0, C.byref(h))
        v = Ints.__new__(Ints)
        v.ctx, v.kind, v.count, v.h = self.ctx, "i64" if signed else "u64", self.n_rows, h
        return v

    def ints_many(self, fields):
        """[(offset, width, signed)] -> one Ints per field, all extracted in ONE pass over the rows (jolt_ints_from_rows_many)"""
        n = len(fields)
        offs = (C.c_size_t * n)(*[f[0] for f in fields])
        widths = (C.c_uint32 * n)(*[f[1] for f in fields])
        signed = (C.c_int32 * n)(*[1 if f[2] else 0 for f in fields])
        hs = (C.c_void_p * n)()
        _call("jolt_ints_from_rows_many", self.ctx, self.ctx.h, self.h, offs, widths, signed, n, hs)
        out = []
        for k, f in enumerate(fields):
            v = Ints.__new__(Ints)
            v.ctx, v.kind, v.count, v.h = self.ctx, "i64" if f[2] else "u64", self.n_rows, C.c_void_p(hs[k])
            out.append(v)
        return out

    def onehot(self, offset, width, shifts, log_k, valid_offset=None):
        sh = (C.c_uint32 * len(shifts))(*shifts)
        h = C.c_void_p()
        vo = valid_offset if valid_offset is not None else 2**64 - 1
        _call("jolt_onehot_from_rows", self.ctx, self.ctx.h, self.h, offset, width, sh, len(shifts), log_k, vo, C.byref(h))
        src = OneHot.__new__(OneHot)
        src.ctx, src.n_polys, src.cycles, src.k, src.h, src.wide = self.ctx, len(shifts), self.n_rows, 1 << log_k, h, log_k > 7
        return src

    def free(self):
        if self.h:
            lib().jolt_rows_free(self.ctx.h, self.h)
            self.h = None


class SplitLt:
    """LT(., r) + constant from split tables, bound low-to-high (optimized/support.rs:640-760)."""

    def __init__(self, ctx, r_cycle, constant=None):
        r = fr(r_cycle).reshape(-1, 4)
        h = C.c_void_p()
        _call("jolt_split_lt_create", ctx, ctx.h, _p(r) if r.shape[0] else None, r.shape[0], _p(fr(constant)) if constant is not None else None, C.byref(h))
        self.ctx, self.h = ctx, h

    def __len__(self):
        n = C.c_size_t()
        _call("jolt_split_lt_len", self.ctx, self.h, C.byref(n))
        return n.value

    def bind(self, r):
        _call("jolt_split_lt_bind", self.ctx, self.ctx.h, self.h, _p(fr(r)))

    def to_dense(self):
        h = C.c_void_p()
        _call("jolt_split_lt_to_dense", self.ctx, self.ctx.h, self.h, C.byref(h))
        return Table(self.ctx, h)

    def final_value(self):
        o = fr_array(1)
        _call("jolt_split_lt_final_value", self.ctx, self.ctx.h, self.h, _p(o))
        return o[0]

    def free(self):
        if self.h:
            lib().jolt_split_lt_free(self.ctx.h, self.h)
            self.h = None


class OneHot:
    """Hot indices of N one-hot selector columns (uint8 [n_polys, cycles], 0xFF = cold cycle) resident on the device."""

    def __init__(self, ctx, indices, k):
        """indices: uint8 (0xFF = cold, k <= 255) or uint16 (0xFFFF = cold: the K = 256 chunks of long traces)"""
        wide = np.asarray(indices).dtype == np.uint16
        idx = np.ascontiguousarray(indices, dtype=np.uint16 if wide else np.uint8)
        assert idx.ndim == 2
        self.ctx, self.n_polys, self.cycles, self.k, self.wide = ctx, idx.shape[0], idx.shape[1], k, wide
        h = C.c_void_p()
        _call("jolt_onehot_upload16" if wide else "jolt_onehot_upload", ctx, ctx.h, idx.ctypes.data_as(C.c_void_p), idx.shape[0], idx.shape[1], k, C.byref(h))
        self.h = h

    def download(self):
        wide = self.wide
        out = np.empty((self.n_polys, self.cycles), dtype=np.uint16 if wide else np.uint8)
        _call("jolt_onehot_download16" if wide else "jolt_onehot_download", self.ctx, self.ctx.h, self.h, out.ctypes.data_as(C.c_void_p))
        return out

    def materialize(self, poly, scale_table):
        h = C.c_void_p()
        _call("jolt_onehot_materialize", self.ctx, self.ctx.h, self.h, poly, scale_table.h, C.byref(h))
        return Table(self.ctx, h)

    def pushforward(self, weights):
        h = C.c_void_p()
        _call("jolt_onehot_pushforward", self.ctx, self.ctx.h, self.h, weights.h, C.byref(h))
        return Table(self.ctx, h)

    def free(self):
        if self.h:
            lib().jolt_onehot_free(self.ctx.h, self.h)
            self.h = None


class Ints:
    """Small machine integers resident on the device for the Dory tier-1 row commitments: uint64 / int64 numpy arrays, or
    i128 as an (n, 2) uint64 array (low, high; two's complement) / a list of Python ints with kind="i128"."""
    KINDS = {"u64": INT_U64, "i64": INT_I64, "i128": INT_I128}

    def __init__(self, ctx, values, kind=None):
        if kind == "i128" and not isinstance(values, np.ndarray):
            values = np.array([[int(v) & (2**64 - 1), (int(v) >> 64) & (2**64 - 1)] for v in values], dtype=np.uint64).reshape(-1, 2)
        v = np.ascontiguousarray(values)
        if kind is None:
            kind = {np.dtype(np.uint64): "u64", np.dtype(np.int64): "i64"}[v.dtype] if v.ndim == 1 else "i128"
        self.ctx, self.kind = ctx, kind
        self.count = v.shape[0]
        h = C.c_void_p()
        _call("jolt_ints_upload", ctx, ctx.h, v.ctypes.data_as(C.c_void_p), self.KINDS[kind], self.count, C.byref(h))
        self.h = h

    def free(self):
        if self.h:
            lib().jolt_ints_free(self.ctx.h, self.h)
            self.h = None


def _dory_commit_rows(self, srs, values, row_width):
    """DoryScheme::feed_u64 / feed_i128 over every row_width window of `values` (an Ints): one G1 point per row."""
    rows = values.count // row_width if row_width else 0
    out = g1_array(max(rows, 1))
    _call("jolt_dory_commit_rows", self, self.h, srs.h, values.h, row_width, _p(out))
    return out[:rows]


def _dory_commit_onehot(self, srs, source, poly, chunk_width):
    """DoryScheme::process_one_hot_chunks_with for hot-index column `poly`: (chunks, k) G1 points."""
    chunks = source.cycles // chunk_width if chunk_width else 0
    out = g1_array(max(chunks * source.k, 1))
    _call("jolt_dory_commit_onehot", self, self.h, srs.h, source.h, poly, chunk_width, _p(out))
    return out[:chunks * source.k].reshape(chunks, source.k, -1)


def _member_lazy_ra_uniform(self, source, scale_tables, V, F, coeffs, w, scale=None, shard_scale=None):
    """eq(w,.) * sum_v coeffs[v] * prod_{i<F} ra_{vF+i}, ra_p(j) = scale_tables[p][index(p,j)], lazily bound (LazyFoldedRa)."""
    w = fr(w).reshape(-1, 4)
    co = np.ascontiguousarray(np.stack([fr(c) for c in coeffs])).reshape(-1, 4)
    st = np.ascontiguousarray(scale_tables, dtype=np.uint64).reshape(-1, 4)
    h = C.c_void_p()
    if shard_scale is not None:
        _call("jolt_member_create_lazy_ra_uniform_sharded", self, self.h, source.h, _p(st), V, F, _p(co), _p(w), w.shape[0], _p(fr(scale)) if scale is not None else None,
              _p(fr(shard_scale)), C.byref(h))
    else:
        _call("jolt_member_create_lazy_ra_uniform", self, self.h, source.h, _p(st), V, F, _p(co), _p(w), w.shape[0], _p(fr(scale)) if scale is not None else None, C.byref(h))
    m = Member(self, h, F + 1, V * F, True, False)
    m.n_evals = F
    m.uniform = True
    m._keepalive = [source]
    return m


def _member_lazy_booleanity(self, source, scale_tables, rho, w, scale=None):
    """eq(w,.) * sum_i (H_i^2 - rho_i H_i), H_i(j) = scale_tables[i][index(i,j)] (gamma-pre-scaled), lazily bound; 2 sums per round."""
    w = fr(w).reshape(-1, 4)
    st = np.ascontiguousarray(scale_tables, dtype=np.uint64).reshape(-1, 4)
    rh = np.ascontiguousarray(np.stack([fr(c) for c in rho])).reshape(-1, 4)
    h = C.c_void_p()
    _call("jolt_member_create_lazy_booleanity", self, self.h, source.h, _p(st), _p(rh), _p(w), w.shape[0], _p(fr(scale)) if scale is not None else None, C.byref(h))
    m = Member(self, h, 3, rh.shape[0], True, False)
    m.n_evals = 2
    m._keepalive = [source]
    return m


Context.member_lazy_booleanity = _member_lazy_booleanity
Context.member_lazy_ra_uniform = _member_lazy_ra_uniform
Context.onehot = lambda self, indices, k: OneHot(self, indices, k)
Context.ints = lambda self, values, kind=None: Ints(self, values, kind)
Context.dory_commit_rows = _dory_commit_rows
Context.dory_commit_onehot = _dory_commit_onehot


# ---- the Dory opening ahead of the pairing rounds (dory.hip): lazy row fold and hint combination
DORY_COMBINE_WINDOW = 5  # kCombineWindow of dory.hip: signed digits of 5 bits


def dory_combine_ops_per_row(n_hints, window=DORY_COMBINE_WINDOW):
    """Upper bound on the group operations one row of dory_combine_hints performs: per window one addition per term, one per magnitude level of the
    running-sum walk, `window` doublings and the Horner addition; (double_and_add = 1.5 * 254 * n_hints is the number it is held against)."""
    windows = (254 + 1 + window - 1) // window
    return windows * (n_hints + (1 << (window - 1)) + window + 1)


def dory_onehot_hint(chunk_commitments):
    """finish_one_hot_column_major_chunks (streaming.rs:318-362): the (chunks, k, 12) output of dory_commit_onehot as the column's hint,
    hint[row * chunks + chunk] = out[chunk * k + row] -- with chunk_width = 2^sigma, row (k << (log_t - sigma)) + chunk of the grid matrix."""
    c = np.asarray(chunk_commitments, dtype=np.uint64)
    return np.ascontiguousarray(c.transpose(1, 0, 2)).reshape(-1, c.shape[2])


def _dory_fold_rows_grid(self, sources, onehot_scalars, dense, dense_scalars, log_k, sigma, left):
    """RlcSource::fold_rows(left, sigma) of the batch's joint polynomial over the 2^log_k x T grid, from the hot indices and dense columns: 2^sigma entries."""
    hs = (C.c_void_p * max(len(sources), 1))(*[s.h for s in sources])
    ds = (C.c_void_p * max(len(dense), 1))(*[t.h for t in dense])
    osc = fr(np.stack([fr(c) for c in onehot_scalars])).reshape(-1, 4) if len(onehot_scalars) else None
    dsc = fr(np.stack([fr(c) for c in dense_scalars])).reshape(-1, 4) if len(dense_scalars) else None
    h = C.c_void_p()
    _call("jolt_dory_fold_rows_grid", self, self.h, hs if sources else None, len(sources), _p(osc), ds if dense else None, len(dense), _p(dsc), log_k, sigma, left.h,
          C.byref(h))
    return Table(self, h)


def _dory_combine_hints(self, hints, scalars):
    """DoryScheme::combine_hints: hints = list of (rows_i, 12) point arrays, scalars = one Fr each; (max rows_i, 12) points."""
    hs = [np.ascontiguousarray(h, dtype=np.uint64).reshape(-1, 12) for h in hints]
    n = len(hs)
    ptrs = (C.c_void_p * max(n, 1))(*[h.ctypes.data for h in hs])
    rows = (C.c_size_t * max(n, 1))(*[h.shape[0] for h in hs])
    sc = fr(np.stack([fr(c) for c in scalars])).reshape(-1, 4) if n else fr_array(1)
    width = max([h.shape[0] for h in hs], default=0)
    out = g1_array(max(width, 1))
    _call("jolt_dory_combine_hints", self, self.h, ptrs, rows, n, _p(sc), _p(out))
    return out[:width]


def host_dory_combine_row(points, scalars):
    """sum_i scalars[i] * points[i] through the per-row routine of dory_combine_hints, on the host"""
    pts = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 12)
    sc = fr(np.stack([fr(c) for c in scalars])).reshape(-1, 4) if pts.shape[0] else fr_array(1)
    out = g1_array(1)
    _call("jolt_host_dory_combine_row", None, _p(pts), _p(sc), pts.shape[0], _p(out))
    return out[0]


# ---- the group and field routines of dory::prove's reduce-and-fold rounds (dory_routines.hip): DoryRoutines<ArkG1> / DoryRoutines<ArkG2>
def g2_array(n):
    """G2 points: (n, 24) uint64 -- Jacobian over Fq2, x.c0, x.c1, y.c0, y.c1, z.c0, z.c1 (ark_bn254::G2Projective)"""
    return np.zeros((n, 24), dtype=np.uint64)


_DORY_GROUPS = {"g1": 12, "g2": 24}


def _dory_pts(group, a):
    return np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, _DORY_GROUPS[group])


def _dory_msm(self, group, bases, scalars):
    """DoryRoutines::msm: sum_i scalars[i] * bases[i] over projective bases; one point"""
    b = _dory_pts(group, bases)
    sc = fr(scalars).reshape(-1, 4)
    if b.shape[0] != sc.shape[0]:
        raise ValueError("msm: bases and scalars differ in length")
    out = np.zeros(_DORY_GROUPS[group], dtype=np.uint64)
    name = f"jolt_dory_{group}_msm"
    _call(name, self, self.h, _p(b) if b.shape[0] else None, _p(sc) if b.shape[0] else None, b.shape[0], _p(out))
    return out


def _dory_fixed_base_mul(self, group, base, scalars):
    """DoryRoutines::fixed_base_vector_scalar_mul: out[i] = scalars[i] * base"""
    b = _dory_pts(group, base)
    sc = fr(scalars).reshape(-1, 4)
    n = sc.shape[0]
    out = np.zeros((max(n, 1), _DORY_GROUPS[group]), dtype=np.uint64)
    name = f"jolt_dory_{group}_fixed_base_mul"
    _call(name, self, self.h, _p(b), _p(sc) if n else None, n, _p(out) if n else None)
    return out[:n]


def _dory_scale_bases_add(self, group, bases, vs, scalar):
    """DoryRoutines::fixed_scalar_mul_bases_then_add: vs[i] + scalar * bases[i]; returns the new vs (the C entry updates its copy in place)"""
    b, v = _dory_pts(group, bases), _dory_pts(group, vs).copy()
    if b.shape[0] != v.shape[0]:
        raise ValueError("lengths must match")
    n = v.shape[0]
    name = f"jolt_dory_{group}_scale_bases_add"
    _call(name, self, self.h, _p(b) if n else None, _p(v) if n else None, n, _p(fr(scalar)))
    return v


def _dory_scale_vs_add(self, group, vs, addends, scalar):
    """DoryRoutines::fixed_scalar_mul_vs_then_add: scalar * vs[i] + addends[i]; returns the new vs"""
    v, a = _dory_pts(group, vs).copy(), _dory_pts(group, addends)
    if a.shape[0] != v.shape[0]:
        raise ValueError("lengths must match")
    n = v.shape[0]
    name = f"jolt_dory_{group}_scale_vs_add"
    _call(name, self, self.h, _p(v) if n else None, _p(a) if n else None, n, _p(fr(scalar)))
    return v


def _dory_fold_field_vectors(self, left, right, scalar):
    """DoryRoutines::fold_field_vectors: left[i] * scalar + right[i]; returns the new left"""
    l, r = fr(left).reshape(-1, 4).copy(), fr(right).reshape(-1, 4)
    if l.shape[0] != r.shape[0]:
        raise ValueError("lengths must match")
    n = l.shape[0]
    _call("jolt_dory_fold_field_vectors", self, self.h, _p(l) if n else None, _p(r) if n else None, n, _p(fr(scalar)))
    return l


def _dory_routines_timing(self, enable):
    """(checks, host -> device, kernels, device -> host) wall ms of the last routine call made while timing was on; then switches timing on / off"""
    ms = (C.c_double * 4)()
    _call("jolt_dory_routines_timing", self, self.h, 1 if enable else 0, ms)
    return tuple(ms)


Context.dory_g1_msm = lambda self, bases, scalars: _dory_msm(self, "g1", bases, scalars)
Context.dory_g2_msm = lambda self, bases, scalars: _dory_msm(self, "g2", bases, scalars)
Context.dory_g1_fixed_base_mul = lambda self, base, scalars: _dory_fixed_base_mul(self, "g1", base, scalars)
Context.dory_g2_fixed_base_mul = lambda self, base, scalars: _dory_fixed_base_mul(self, "g2", base, scalars)
Context.dory_g1_scale_bases_add = lambda self, bases, vs, scalar: _dory_scale_bases_add(self, "g1", bases, vs, scalar)
Context.dory_g2_scale_bases_add = lambda self, bases, vs, scalar: _dory_scale_bases_add(self, "g2", bases, vs, scalar)
Context.dory_g1_scale_vs_add = lambda self, vs, addends, scalar: _dory_scale_vs_add(self, "g1", vs, addends, scalar)
Context.dory_g2_scale_vs_add = lambda self, vs, addends, scalar: _dory_scale_vs_add(self, "g2", vs, addends, scalar)
Context.dory_fold_field_vectors = _dory_fold_field_vectors
Context.dory_routines_timing = _dory_routines_timing



def host_fq2_op(op, a, b=None):
    """Fq2 on the host as the kernels compute it; a, b = (8,) uint64 (c0, c1); raises JoltError(1) for an operand that is not canonical"""
    a = np.ascontiguousarray(a, dtype=np.uint64).reshape(8)
    b = np.ascontiguousarray(b, dtype=np.uint64).reshape(8) if b is not None else None
    out = np.zeros(8, dtype=np.uint64)
    _call("jolt_host_fq2_op", None, op, _p(a), _p(b), _p(out))
    return out


def _host_g2(name, *pts):
    out = np.zeros(24, dtype=np.uint64)
    args = [_p(np.ascontiguousarray(p, dtype=np.uint64)) for p in pts]
    _call(name, None, *args, _p(out))
    return out


def host_g2_add(p, q): return _host_g2("jolt_host_g2_add", p, q)
def host_g2_double(p): return _host_g2("jolt_host_g2_double", p)
def host_g2_neg(p): return _host_g2("jolt_host_g2_neg", p)
def host_g2_scalar_mul(p, s): return _host_g2("jolt_host_g2_scalar_mul", p, s)


def host_g2_eq(p, q):
    e = C.c_int32()
    _call("jolt_host_g2_eq", None, _p(np.ascontiguousarray(p, dtype=np.uint64)), _p(np.ascontiguousarray(q, dtype=np.uint64)), C.byref(e))
    return bool(e.value)


def host_g2_is_on_curve(p):
    e = C.c_int32()
    _call("jolt_host_g2_is_on_curve", None, _p(np.ascontiguousarray(p, dtype=np.uint64)), C.byref(e))
    return bool(e.value)


def _host_dory_one(name, group, *args):
    out = np.zeros(_DORY_GROUPS[group], dtype=np.uint64)
    _call(name, None, *[_p(np.ascontiguousarray(a, dtype=np.uint64)) for a in args], _p(out))
    return out


def host_dory_scale_add_one(group, scaled, addend, scalar):
    """addend + scalar * scaled: one element of both shared-scalar routines through the lanes' code (non-adjacent form and its walk), on the host"""
    return _host_dory_one(f"jolt_host_dory_{group}_scale_add_one", group, scaled, addend, scalar)


def host_dory_fixed_base_one(group, base, scalar):
    """scalar * base through the fixed-base table and window walk of the device lanes, on the host"""
    return _host_dory_one(f"jolt_host_dory_{group}_fixed_base_one", group, base, scalar)


def host_dory_msm_term(group, base, scalar):
    """scalar * base as one MSM term of the device lanes, on the host"""
    return _host_dory_one(f"jolt_host_dory_{group}_msm_term", group, base, scalar)


# ---- Dory's multi-pairings (dory_pairing.hip): the tier-2 commitment and the multi-pairings of the reduce-and-fold rounds


def gt_array():
    """one GT element: (48,) uint64 -- twelve Montgomery Fq, c0.c0.c0, c0.c0.c1, c0.c1.c0, ..., c1.c2.c1 (ark_bn254::Fq12)"""
    return np.zeros(48, dtype=np.uint64)


def _pair_g1(g1s):
    return np.ascontiguousarray(g1s, dtype=np.uint64).reshape(-1, 12)


def _dory_multi_pair(self, g1s, g2s, final_exponentiation=True):
    """prod_i e(g1s[i], g2s[i]) (PairingGroup::multi_pairing, dory's multi_pair); final_exponentiation=False: the raw Miller product"""
    a, b = _pair_g1(g1s), _dory_pts("g2", g2s)
    if a.shape[0] != b.shape[0]:
        raise ValueError("multi_pair: the two sides differ in length")
    n, out = a.shape[0], gt_array()
    name = "jolt_dory_multi_pair" if final_exponentiation else "jolt_dory_multi_miller"
    _call(name, self, self.h, _p(a) if n else None, _p(b) if n else None, n, _p(out))
    return out


class G2Prepared:
    """the line tables of n G2 points, resident on the device (jolt_dory_g2_prepare)"""

    def __init__(self, ctx, h, n):
        self.ctx, self.h, self.n = ctx, h, n

    def free(self):
        if self.h:
            _call("jolt_g2_prepared_free", self.ctx, self.ctx.h, self.h)
            self.h = None


def _dory_g2_prepare(self, g2s):
    b = _dory_pts("g2", g2s)
    h = C.c_void_p()
    _call("jolt_dory_g2_prepare", self, self.h, _p(b) if b.shape[0] else None, b.shape[0], C.byref(h))
    return G2Prepared(self, h, b.shape[0])


def _dory_multi_pair_g2_setup(self, g1s, prepared, n=None):
    """prod_{i < n} e(g1s[i], prepared point i) (dory's multi_pair_g2_setup over srs_prefix); n defaults to len(g1s)"""
    a = _pair_g1(g1s)
    n = a.shape[0] if n is None else n
    out = gt_array()
    _call("jolt_dory_multi_pair_g2_setup", self, self.h, _p(a) if a.shape[0] else None, prepared.h, n, _p(out))
    return out


def _dory_pairing_timing(self, enable):
    """(checks, host -> device, prepare, Miller, product, device -> host, final exponentiation) wall ms of the last pairing call made while timing was on"""
    ms = (C.c_double * 7)()
    _call("jolt_dory_pairing_timing", self, self.h, 1 if enable else 0, ms)
    return tuple(ms)


Context.dory_multi_pair = _dory_multi_pair
Context.dory_g2_prepare = _dory_g2_prepare
Context.dory_multi_pair_g2_setup = _dory_multi_pair_g2_setup
Context.dory_pairing_timing = _dory_pairing_timing


# ---- Dory's rounds on resident vectors (dory_resident.hip): vectors that stay in HBM, in-place routines on views, product batches
_DORY_KIND_WIDTH = {DORY_KIND_G1: 12, DORY_KIND_G2: 24, DORY_KIND_FR: 4}
_DORY_RESULT_WIDTH = {DORY_PAIR: 48, DORY_MSM_G1: 12, DORY_MSM_G2: 24}


class DoryItem(C.Structure):
    """jolt_dory_item"""
    _fields_ = [("op", C.c_int32), ("a", C.c_void_p), ("a_first", C.c_size_t), ("b", C.c_void_p), ("b_first", C.c_size_t),
                ("prepared", C.c_void_p), ("prepared_first", C.c_size_t), ("n", C.c_size_t)]


class DoryVec:
    """A G1 / G2 / Fr array resident on the device (jolt_dory_vec); its elements were checked when it was uploaded.  v.view(first, n) names a range of it."""

    def __init__(self, ctx, h, kind):
        self.ctx, self.h, self.kind = ctx, h, kind

    def __len__(self):
        n = C.c_size_t()
        _call("jolt_dory_vec_len", self.ctx, self.h, C.byref(n))
        return n.value

    def view(self, first=0, n=None):
        return (self, first, len(self) - first if n is None else n)

    def device_kind(self):
        """the kind the library holds for the handle"""
        k = C.c_int32()
        _call("jolt_dory_vec_kind", self.ctx, self.h, C.byref(k))
        return k.value

    def download(self, first=0, n=None):
        n = len(self) - first if n is None else n
        out = np.zeros((n, _DORY_KIND_WIDTH[self.kind]), dtype=np.uint64)
        _call("jolt_dory_vec_download", self.ctx, self.ctx.h, self.h, first, n, _p(out) if n else None)
        return out

    def truncate(self, n):
        _call("jolt_dory_vec_truncate", self.ctx, self.h, n)

    def free(self):
        if self.h:
            _call("jolt_dory_vec_free", self.ctx, self.ctx.h, self.h)
            self.h = None


def _dory_view(v):
    """a DoryVec (all of it) or (DoryVec, first, n)"""
    return v.view() if isinstance(v, DoryVec) else v


def _dory_vec_upload(self, kind, host):
    a = np.ascontiguousarray(host, dtype=np.uint64).reshape(-1, _DORY_KIND_WIDTH[kind])
    h = C.c_void_p()
    _call("jolt_dory_vec_upload", self, self.h, kind, _p(a) if a.shape[0] else None, a.shape[0], C.byref(h))
    return DoryVec(self, h, kind)


def _dory_g2_prepare_vec(self, view):
    """the line table of a resident G2 view, built on the device (jolt_dory_g2_prepare_vec)"""
    v, first, n = _dory_view(view)
    h = C.c_void_p()
    _call("jolt_dory_g2_prepare_vec", self, self.h, v.h, first, n, C.byref(h))
    return G2Prepared(self, h, n)


def _dory_two_views(x, y):
    (xv, xf, xn), (yv, yf, yn) = _dory_view(x), _dory_view(y)
    if xn != yn:
        raise ValueError("the two views differ in length")
    return xv, xf, yv, yf, xn


def _dory_vec_scale_bases_add(self, bases, vs, scalar):
    """vs[i] += scalar * bases[i] in place on views (fixed_scalar_mul_bases_then_add); enqueued, not awaited"""
    bv, bf, vv, vf, n = _dory_two_views(bases, vs)
    _call("jolt_dory_vec_scale_bases_add", self, self.h, bv.h, bf, vv.h, vf, n, _p(fr(scalar)))


def _dory_vec_scale_vs_add(self, vs, addends, scalar):
    """vs[i] = scalar * vs[i] + addends[i] in place on views (fixed_scalar_mul_vs_then_add); enqueued, not awaited"""
    vv, vf, av, af, n = _dory_two_views(vs, addends)
    _call("jolt_dory_vec_scale_vs_add", self, self.h, vv.h, vf, av.h, af, n, _p(fr(scalar)))


def _dory_vec_fold_field(self, left, right, scalar):
    """left[i] = left[i] * scalar + right[i] in place on Fr views (fold_field_vectors); enqueued, not awaited"""
    lv, lf, rv, rf, n = _dory_two_views(left, right)
    _call("jolt_dory_vec_fold_field", self, self.h, lv.h, lf, rv.h, rf, n, _p(fr(scalar)))


def _dory_state_alloc(self, kind, n):
    """n neutral elements on the device (jolt_dory_state_alloc): identities (1, 1, 0), or zeros for DORY_KIND_FR; enqueued, not awaited"""
    h = C.c_void_p()
    _call("jolt_dory_state_alloc", self, self.h, kind, n, C.byref(h))
    return DoryVec(self, h, kind)


def _dory_state_from_table(self, table, dst, table_first=0):
    """dst[i] = table[table_first + i] over the Fr view dst = DoryVec or (DoryVec, first, n): a device copy (jolt_dory_state_from_table); enqueued, not awaited"""
    dv, df, n = _dory_view(dst)
    _call("jolt_dory_state_from_table", self, self.h, table.h, table_first, dv.h, df, n)


def _dory_state_combine_hints(self, hints, scalars, out, out_first=0):
    """DoryScheme::combine_hints on resident G1 views: out[out_first + row] = sum_i scalars[i] * hints[i][row], hints = DoryVec or (DoryVec, first, rows) each
    (jolt_dory_state_combine_hints); the number of rows written, max_i rows_i"""
    views = [_dory_view(h) for h in hints]
    n = len(views)
    hs, firsts, rows = _dory_view_arrays(views)
    sc = fr(np.stack([fr(c) for c in scalars])).reshape(-1, 4) if n else fr_array(1)
    if sc.shape[0] != max(n, 1):
        raise ValueError("one scalar per hint")
    _call("jolt_dory_state_combine_hints", self, self.h, hs, firsts, rows, n, _p(sc), out.h, out_first)
    return max([r for _, _, r in views], default=0)


def _dory_state_fixed_base_mul(self, kind, base, scalars, out):
    """out[i] = scalars[i] * base on views (fixed_base_vector_scalar_mul): kind = DORY_KIND_G1 / _G2, base one host point, scalars an Fr view, out a view of `kind`"""
    b = np.ascontiguousarray(base, dtype=np.uint64).reshape(_DORY_KIND_WIDTH[kind])
    sv, sf, ov, of, n = _dory_two_views(scalars, out)
    _call("jolt_dory_state_fixed_base_mul", self, self.h, kind, _p(b), sv.h, sf, ov.h, of, n)


def dory_item(op, a, b, prepared_first=0):
    """one item of a product batch: a, b = DoryVec or (DoryVec, first, n); for DORY_PAIR b may be a G2Prepared, read from point prepared_first on"""
    av, af, n = _dory_view(a)
    if isinstance(b, G2Prepared):
        return DoryItem(op, av.h, af, None, 0, b.h, prepared_first, n)
    bv, bf, bn = _dory_view(b)
    if bn != n:
        raise ValueError("the two views of an item differ in length")
    return DoryItem(op, av.h, af, bv.h, bf, None, 0, n)


def _dory_products(self, items):
    """jolt_dory_products: every item (dory_item) of the list in one launch set; one (48,) GT, (12,) G1 or (24,) G2 array per item"""
    n = len(items)
    arr = (DoryItem * max(n, 1))(*items)
    outs = np.zeros((max(n, 1), 48), dtype=np.uint64)
    _call("jolt_dory_products", self, self.h, arr if n else None, n, _p(outs) if n else None)
    return [outs[k, :_DORY_RESULT_WIDTH[items[k].op]].copy() for k in range(n)]


def host_dory_batch_plan(lens):
    """the launch plan of one chain of a product batch (dory_batch_plan.hpp): (wg_item, wg_first, item_base, levels)"""
    n = len(lens)
    a = (C.c_size_t * max(n, 1))(*lens)
    base = (C.c_size_t * max(n, 1))()
    n_wgs, levels = C.c_size_t(), C.c_uint32()
    _call("jolt_host_dory_batch_plan", None, a, n, 0, None, None, base, C.byref(n_wgs), C.byref(levels))
    w = n_wgs.value
    wg_item, wg_first = np.zeros(max(w, 1), dtype=np.uint32), np.zeros(max(w, 1), dtype=np.uint32)
    _call("jolt_host_dory_batch_plan", None, a, n, max(w, 1), _p(wg_item), _p(wg_first), base, C.byref(n_wgs), C.byref(levels))
    return wg_item[:w], wg_first[:w], [int(b) for b in base[:n]], levels.value


Context.dory_vec_upload = _dory_vec_upload
Context.dory_g2_prepare_vec = _dory_g2_prepare_vec
Context.dory_vec_scale_bases_add = _dory_vec_scale_bases_add
Context.dory_vec_scale_vs_add = _dory_vec_scale_vs_add
Context.dory_vec_fold_field = _dory_vec_fold_field
Context.dory_products = _dory_products
Context.dory_state_alloc = _dory_state_alloc
Context.dory_state_from_table = _dory_state_from_table
Context.dory_state_combine_hints = _dory_state_combine_hints
Context.dory_state_fixed_base_mul = _dory_state_fixed_base_mul


# ---- Dory evaluation proofs as one call (dory_scheme.hip): the setup object, a round's update as one call, the opening under Fiat-Shamir, the byte forms
DORY_TRANSCRIPT_FN = abi.CALLBACK_TYPES["jolt_dory_transcript_fn"]


def _dory_view_arrays(views):
    n = len(views)
    hs = (C.c_void_p * max(n, 1))(*[v.h for v, _, _ in views])
    firsts = (C.c_size_t * max(n, 1))(*[f for _, f, _ in views])
    rows = (C.c_size_t * max(n, 1))(*[r for _, _, r in views])
    return hs, firsts, rows


class DoryLibSetup:
    """jolt_dory_setup: Gamma1, Gamma2 (resident, checked once), Gamma2's prepared table, H1 and H2 behind one handle of the library"""

    def __init__(self, ctx, gamma1, gamma2, h1, h2):
        g1 = np.ascontiguousarray(gamma1, dtype=np.uint64).reshape(-1, 12)
        g2 = np.ascontiguousarray(gamma2, dtype=np.uint64).reshape(-1, 24)
        if g1.shape[0] != g2.shape[0]:
            raise ValueError("Gamma1 and Gamma2 have one length, a power of two")
        self.ctx, self.h = ctx, C.c_void_p()
        self.h1 = np.ascontiguousarray(h1, dtype=np.uint64).reshape(12).copy()
        self.h2 = np.ascontiguousarray(h2, dtype=np.uint64).reshape(24).copy()
        _call("jolt_dory_setup_create", ctx, ctx.h, _p(g1), _p(g2), g1.shape[0], _p(self.h1), _p(self.h2), C.byref(self.h))
        n = C.c_size_t()
        _call("jolt_dory_setup_size", ctx, self.h, C.byref(n))
        self.n = n.value

    def tier2(self, hints):
        """the tier-2 commitments of resident G1 views (DoryVec or (DoryVec, first, rows)): one product batch (jolt_dory_setup_tier2); one (48,) GT each"""
        views = [_dory_view(h) for h in hints]
        hs, firsts, rows = _dory_view_arrays(views)
        outs = np.zeros((max(len(views), 1), 48), dtype=np.uint64)
        _call("jolt_dory_setup_tier2", self.ctx, self.ctx.h, self.h, hs, firsts, rows, len(views), _p(outs))
        return [outs[k].copy() for k in range(len(views))]

    _verifier = None

    def verifier(self):
        """the verifier's precomputed GT values (DoryVerifierSetup), built once -- one product batch over the resident bases -- and closed with the setup"""
        if self._verifier is None:
            self._verifier = DoryVerifierSetup(self)
        return self._verifier

    def combine(self, commitments, scalars):
        """DoryScheme::combine: prod_i commitments[i]^scalars[i] in GT, one multi-exponentiation on the device (jolt_dory_gt_multi_exp)"""
        return self.ctx.dory_gt_multi_exp(commitments, scalars)

    def close(self):
        if self._verifier is not None:
            self._verifier.close()
            self._verifier = None
        if self.h:
            _call("jolt_dory_setup_free", self.ctx, self.ctx.h, self.h)
            self.h = None

    free = close


def _dory_round_update(self, mode, v1, v2, a, b, scalar, scalar_inv):
    """jolt_dory_round_update: one of a round's two in-place updates as one call, the G1 work beside the G2 work; enqueued, not awaited.  Views of one length n:
    DORY_UPDATE_BETA   v1 += scalar * a, v2 += scalar_inv * b with a, b = views of Gamma1, Gamma2
    DORY_UPDATE_ALPHA  v1, a = s1 folded under scalar, v2, b = s2 under scalar_inv; the four vectors are truncated to first + n / 2"""
    views = [_dory_view(x) for x in (v1, v2, a, b)]
    if len({n for _, _, n in views}) != 1:
        raise ValueError("the four views of a round update have one length")
    (v1v, v1f, n), (v2v, v2f, _), (av, af, _), (bv, bf, _) = views
    _call("jolt_dory_round_update", self, self.h, mode, v1v.h, v1f, v2v.h, v2f, av.h, af, bv.h, bf, n, _p(fr(scalar)), _p(fr(scalar_inv)))


def host_dory_proof_counts(sigma):
    """(GT elements, G1 points, G2 points, challenges) of an opening of 2^sigma columns (jolt_host_dory_proof_counts)"""
    c = [C.c_size_t() for _ in range(4)]
    _call("jolt_host_dory_proof_counts", None, sigma, *[C.byref(x) for x in c])
    return tuple(x.value for x in c)


def _dory_open(self, setup, hints, scalars, v_table, left, right, nu, sigma, transcript=None, callback=None):
    """One evaluation proof in one call: jolt_host_dory_open under `transcript` (a HostTranscript), or jolt_host_dory_open_with_transcript under
    callback(phase, round, gts (k, 48), g1s (k, 12), g2s (k, 24)) -> the (4,) challenge after that message (None for DORY_PHASE_VMV / _FINAL) or an int status that
    aborts the opening.  dict(gts, g1s, g2s, challenges) in protocol order."""
    if (transcript is None) == (callback is None):
        raise ValueError("an opening runs under a transcript or under a callback")
    views = [_dory_view(h) for h in hints]
    hs, firsts, rows = _dory_view_arrays(views)
    sc = fr(np.stack([fr(c).reshape(4) for c in scalars])) if len(scalars) else fr_array(1)
    if sc.shape[0] != max(len(views), 1) or len(scalars) != len(views):
        raise ValueError("one scalar per hint")
    n_gt, n_g1, n_g2, n_ch = host_dory_proof_counts(sigma)
    gts, g1s, g2s, ch = np.zeros((n_gt, 48), dtype=np.uint64), np.zeros((n_g1, 12), dtype=np.uint64), np.zeros((n_g2, 24), dtype=np.uint64), fr_array(n_ch)
    head = (self.h, setup.h, hs, firsts, rows, len(views), _p(sc), v_table.h, left.h, right.h, nu, sigma)
    tail = (_p(gts), _p(g1s), _p(g2s), _p(ch))
    if transcript is not None:
        _call("jolt_host_dory_open", self, *head, transcript.h, *tail)
    else:
        err = []

        def cb(user, phase, rnd, p_gt, k_gt, p_g1, k_g1, p_g2, k_g2, out):
            try:
                take = lambda p, k, w: np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint64)), shape=(k, w)).copy() if k else np.zeros((0, w), dtype=np.uint64)  # noqa: E731
                c = callback(phase, rnd, take(p_gt, k_gt, 48), take(p_g1, k_g1, 12), take(p_g2, k_g2, 24))
                if isinstance(c, (int, np.integer)) and not isinstance(c, bool):
                    return int(c)
                if c is not None:
                    c = np.ascontiguousarray(c, dtype=np.uint64).reshape(4)
                    C.memmove(out, c.ctypes.data, 32)
                return 0
            except Exception as e:  # never unwind through the C frame
                err.append(e)
                return 4

        fn = DORY_TRANSCRIPT_FN(cb)
        st = lib().jolt_host_dory_open_with_transcript(*head, fn, None, *tail)
        if err:
            raise err[0]
        _ck(st, "jolt_host_dory_open_with_transcript", self)
    return dict(gts=gts, g1s=g1s, g2s=g2s, challenges=ch)


def host_g2_serialize_compressed(p):
    out = (C.c_uint8 * 64)()
    _call("jolt_host_g2_serialize_compressed", None, _p(np.ascontiguousarray(p, dtype=np.uint64)), out)
    return bytes(out)


def host_gt_serialize(f):
    out = (C.c_uint8 * 384)()
    _call("jolt_host_gt_serialize", None, _p(np.ascontiguousarray(f, dtype=np.uint64)), out)
    return bytes(out)


def host_dory_transcript_append(transcript, element):
    """one group element as JoltToDoryTranscript::append_group absorbs it; the kind by the element's width: (48,) GT, (12,) G1, (24,) G2"""
    e = np.ascontiguousarray(element, dtype=np.uint64).reshape(-1)
    if e.size == 48:
        _call("jolt_host_dory_transcript_append_gt", None, transcript.h, _p(e))
    elif e.size == 12:
        _call("jolt_host_dory_transcript_append_g1", None, transcript.h, _p(e))
    elif e.size == 24:
        _call("jolt_host_dory_transcript_append_g2", None, transcript.h, _p(e))
    else:
        raise ValueError("a GT element has 48 words, a G1 point 12, a G2 point 24")


def host_opening_statement_absorb(transcript, evaluations):
    """the statement of HomomorphicBatch::prove_batch into `transcript` (jolt_host_opening_statement_absorb): LabelWithCount(b"rlc_claims", n) and the n evaluations;
    -> (n, 4) the RLC scalars 1, gamma, ..., gamma^(n - 1) of the ONE challenge_scalar that follows"""
    v = fr(evaluations).reshape(-1, 4)
    out = fr_array(max(v.shape[0], 1))
    _call("jolt_host_opening_statement_absorb", None, transcript.h, _p(v), v.shape[0], _p(out))
    return out[:v.shape[0]]


def host_opening_claim_absorb(transcript, point, value):
    """the closing claim (jolt_host_opening_claim_absorb): LabelWithCount(b"opening_point", len(point)), the coordinates in order, Label(b"opening_eval"), the value"""
    p = fr(point).reshape(-1, 4)
    _call("jolt_host_opening_claim_absorb", None, transcript.h, _p(p) if p.shape[0] else None, p.shape[0], _p(fr(value).reshape(4)))


DORY_ORDERS = {"cycle_major": 0, "address_major": 1}  # JOLT_DORY_ORDER_* of the header


def _dory_prove_batch(self, setup, hints, evaluations, sources, dense, log_k, point, transcript, column_of_claim=None, blocks=(), block_sigmas=(), order="cycle_major",
                      log_extra=0):
    """HomomorphicBatch::<DoryScheme>::prove_batch as one call (jolt_host_dory_prove_batch): setup a DoryLibSetup; hints one resident G1 view per claim; evaluations
    (n, 4) as the statement holds them; sources / dense / log_k the joint polynomial's columns as dory_fold_rows_grid takes them; column_of_claim[i] = claim i's column
    in that order (None: the identity); point: log_k + log T coordinates, most significant first; transcript a HostTranscript.
    blocks / block_sigmas / order / log_extra (any of them given: jolt_host_dory_prove_batch_blocks): block-embedded Tables of 2^m field elements with their sigma_d, as
    dory_fold_rows_blocks takes them -- the columns after the dense ones; order "cycle_major" or "address_major" (the trace as dory_fold_rows_grid_am places it, log_block
    = log_k + log_extra, log_stride = log_extra; the point is then log T + log_k + log_extra coordinates in grid order).  Without them the call is the call it was.
    -> dict(gts, g1s, g2s, challenges, scalars, joint_eval, nu, sigma): the proof in protocol order, the RLC scalars 1, gamma, ... and sum_i scalars[i] evaluations[i]."""
    views = [_dory_view(h) for h in hints]
    hs, firsts, rows = _dory_view_arrays(views)
    ev = fr(evaluations).reshape(-1, 4)
    if ev.shape[0] != len(views):
        raise ValueError("one evaluation per hint")
    pt = fr(point).reshape(-1, 4)
    sigma = (pt.shape[0] + 1) // 2
    n_gt, n_g1, n_g2, n_ch = host_dory_proof_counts(sigma)
    gts, g1s, g2s, ch = np.zeros((n_gt, 48), dtype=np.uint64), np.zeros((n_g1, 12), dtype=np.uint64), np.zeros((n_g2, 24), dtype=np.uint64), fr_array(n_ch)
    scalars, joint = fr_array(max(len(views), 1)), fr_array(1)
    ss = (C.c_void_p * max(len(sources), 1))(*[s.h for s in sources])
    ds = (C.c_void_p * max(len(dense), 1))(*[t.h for t in dense])
    claim_order = None if column_of_claim is None else (C.c_size_t * max(len(column_of_claim), 1))(*[int(c) for c in column_of_claim])
    if claim_order is not None and len(column_of_claim) != len(views):
        raise ValueError("one column per claim")
    if order not in DORY_ORDERS:
        raise ValueError("order is cycle_major or address_major")
    if len(block_sigmas) != len(blocks):
        raise ValueError("one sigma per block")
    if not blocks and order == "cycle_major" and log_extra == 0:
        _call("jolt_host_dory_prove_batch", self, self.h, setup.h, hs, firsts, rows, len(views), _p(ev), ss if sources else None, len(sources), ds if dense else None,
              len(dense), log_k, claim_order, _p(pt), pt.shape[0], transcript.h, _p(gts), _p(g1s), _p(g2s), _p(ch), _p(scalars), _p(joint))
    else:
        bs = (C.c_void_p * max(len(blocks), 1))(*[t.h for t in blocks])
        sg = (C.c_uint32 * max(len(blocks), 1))(*[int(x) for x in block_sigmas])
        _call("jolt_host_dory_prove_batch_blocks", self, self.h, setup.h, hs, firsts, rows, len(views), _p(ev), ss if sources else None, len(sources),
              ds if dense else None, len(dense), bs if blocks else None, sg if blocks else None, len(blocks), log_k, DORY_ORDERS[order], log_extra, claim_order, _p(pt),
              pt.shape[0], transcript.h, _p(gts), _p(g1s), _p(g2s), _p(ch), _p(scalars), _p(joint))
    return dict(gts=gts, g1s=g1s, g2s=g2s, challenges=ch, scalars=scalars[:len(views)], joint_eval=joint[0], nu=pt.shape[0] - sigma, sigma=sigma)


def _grid_evaluate_columns(self, sources, dense, log_k, point):
    """the statement's claims from one pass over the witness (jolt_grid_evaluate_columns): (columns, 4), the multilinear evaluation at `point` of every column of the
    cycle-major grid, in dory_fold_rows_grid's column order (one-hot columns source by source, then dense)"""
    pt = fr(point).reshape(-1, 4)
    n = sum(s.n_polys for s in sources) + len(dense)
    out = fr_array(max(n, 1))
    ss = (C.c_void_p * max(len(sources), 1))(*[s.h for s in sources])
    ds = (C.c_void_p * max(len(dense), 1))(*[t.h for t in dense])
    _call("jolt_grid_evaluate_columns", self, self.h, ss if sources else None, len(sources), ds if dense else None, len(dense), log_k, _p(pt), pt.shape[0], _p(out))
    return out[:n]


Context.dory_setup_create = lambda self, gamma1, gamma2, h1, h2: DoryLibSetup(self, gamma1, gamma2, h1, h2)
Context.dory_round_update = _dory_round_update
Context.dory_open = _dory_open
Context.dory_prove_batch = _dory_prove_batch
Context.grid_evaluate_columns = _grid_evaluate_columns


# ---- Dory verification (dory_verify.hip): GT multi-exponentiation, the verifier's precomputed GT values, the verifier as one call
def _gt_rows(gts):
    return np.ascontiguousarray(gts, dtype=np.uint64).reshape(-1, 48)


def _gt_powers_in(gts, scalars):
    g, s = _gt_rows(gts), fr(scalars).reshape(-1, 4)
    if g.shape[0] != s.shape[0]:
        raise ValueError("one scalar per GT element")
    return g, s, g.shape[0]


def _dory_gt_pow_many(self, gts, scalars):
    """(n, 48): gts[i]^scalars[i], n independent powers in one launch (jolt_dory_gt_pow_many); any canonical Fq12 is a valid base"""
    g, s, n = _gt_powers_in(gts, scalars)
    out = np.zeros((n, 48), dtype=np.uint64)
    _call("jolt_dory_gt_pow_many", self, self.h, _p(g) if n else None, _p(s) if n else None, n, _p(out) if n else None)
    return out


def _dory_gt_multi_exp(self, gts, scalars):
    """(48,): prod_i gts[i]^scalars[i] (DoryScheme::combine, jolt_dory_gt_multi_exp); one for no terms"""
    g, s, n = _gt_powers_in(gts, scalars)
    out = gt_array()
    _call("jolt_dory_gt_multi_exp", self, self.h, _p(g) if n else None, _p(s) if n else None, n, _p(out))
    return out


class DoryVerifierSetup:
    """jolt_dory_verifier_setup: the 3 log2(n) + 4 GT values a verifier holds for a DoryLibSetup of n bases, from one product batch"""

    def __init__(self, setup):
        self.ctx, self.setup, self.h = setup.ctx, setup, C.c_void_p()
        _call("jolt_dory_verifier_setup_create", self.ctx, self.ctx.h, setup.h, C.byref(self.h))

    def values(self):
        """(3 s + 4, 48): chi_0 .. chi_s, Delta1R_0 .. Delta1R_{s-1}, Delta2R_0 .. Delta2R_{s-1}, HT, e(H1, Gamma2[0]), e(Gamma1[0], H2)"""
        out = np.zeros((3 * (self.setup.n.bit_length() - 1) + 4, 48), dtype=np.uint64)
        _call("jolt_dory_verifier_setup_values", self.ctx, self.h, _p(out))
        return out

    def timing(self, enable):
        """(host replay + exponents, group folds, pairings + final exponentiations, multi-exponentiation) wall ms of the last verification made while timing was on"""
        ms = (C.c_double * 4)()
        _call("jolt_dory_verifier_setup_timing", self.ctx, self.h, 1 if enable else 0, ms)
        return tuple(ms)

    def close(self):
        if self.h:
            _call("jolt_dory_verifier_setup_free", self.ctx, self.ctx.h, self.h)
            self.h = None

    free = close


def host_dory_verify_exponents(sigma, challenges, d, s1, s2, y):
    """jolt_host_dory_verify_exponents: dict(proof_gt (2 + 6 sigma, 4), commitment (4,), setup (3 sigma + 4, 4), g1 (1 + 3 sigma, 4), g2 (3 sigma, 4), h2 (4,))"""
    ch = fr(challenges).reshape(-1, 4)
    if ch.shape[0] != 2 * sigma + 1:
        raise ValueError("beta_k, alpha_k per round and gamma: 2 sigma + 1 challenges")
    outs = [fr_array(2 + 6 * sigma), fr_array(1), fr_array(3 * sigma + 4), fr_array(1 + 3 * sigma), fr_array(max(3 * sigma, 1)), fr_array(1)]
    _call("jolt_host_dory_verify_exponents", None, sigma, _p(ch), *[_p(fr(x).reshape(4)) for x in (d, s1, s2, y)], *[_p(o) for o in outs])
    return dict(proof_gt=outs[0], commitment=outs[1][0], setup=outs[2], g1=outs[3], g2=outs[4][:3 * sigma], h2=outs[5][0])


def _dory_verify(self, verifier, commitment, y, left, right, nu, sigma, proof, transcript=None, callback=None):
    """DoryScheme::verify as one call (jolt_host_dory_verify under a HostTranscript, jolt_host_dory_verify_with_transcript under a callback of dory_open's shape, which
    is also asked for d with DORY_PHASE_D).  verifier a DoryVerifierSetup; left (2^nu, 4), right (2^sigma, 4) host arrays; proof a dict(gts, g1s, g2s) as dory_open
    returns.  -> (accepted, failed_check): failed_check 0 none, 1 the VMV check, 2 the final check.  A rejected proof raises nothing."""
    if (transcript is None) == (callback is None):
        raise ValueError("a verification runs under a transcript or under a callback")
    lt, rt = fr(left).reshape(-1, 4), fr(right).reshape(-1, 4)
    if nu > 62 or sigma > 62 or lt.shape[0] != 1 << nu or rt.shape[0] != 1 << sigma:
        raise ValueError("left has 2^nu entries, right has 2^sigma")
    n_gt, n_g1, n_g2, _ = host_dory_proof_counts(sigma)
    gts, g1s, g2s = _gt_rows(proof["gts"]), _pair_g1(proof["g1s"]), _dory_pts("g2", proof["g2s"])
    if (gts.shape[0], g1s.shape[0], g2s.shape[0]) != (n_gt, n_g1, n_g2):
        raise ValueError("the proof does not have the element counts of an opening of 2^sigma columns")
    accepted, failed = C.c_int32(-1), C.c_int32(-1)
    head = (self.h, verifier.h, verifier.setup.h, _p(_gt_rows(commitment).reshape(48)), _p(fr(y).reshape(4)), _p(lt), _p(rt), nu, sigma, _p(gts), _p(g1s), _p(g2s))
    if transcript is not None:
        _call("jolt_host_dory_verify", self, *head, transcript.h, C.byref(accepted), C.byref(failed))
    else:
        err = []

        def cb(user, phase, rnd, p_gt, k_gt, p_g1, k_g1, p_g2, k_g2, out):
            try:
                take = lambda p, k, w: np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint64)), shape=(k, w)).copy() if k else np.zeros((0, w), dtype=np.uint64)  # noqa: E731
                c = callback(phase, rnd, take(p_gt, k_gt, 48), take(p_g1, k_g1, 12), take(p_g2, k_g2, 24))
                if isinstance(c, (int, np.integer)) and not isinstance(c, bool):
                    return int(c)
                if c is not None:
                    c = np.ascontiguousarray(c, dtype=np.uint64).reshape(4)
                    C.memmove(out, c.ctypes.data, 32)
                return 0
            except Exception as e:  # never unwind through the C frame
                err.append(e)
                return 4

        fn = DORY_TRANSCRIPT_FN(cb)
        st = lib().jolt_host_dory_verify_with_transcript(*head, fn, None, C.byref(accepted), C.byref(failed))
        if err:
            raise err[0]
        _ck(st, "jolt_host_dory_verify_with_transcript", self)
    return bool(accepted.value), failed.value


def _dory_verify_batch(self, verifier, commitments, evaluations, point, proof, transcript):
    """HomomorphicBatch::<DoryScheme>::verify_batch as one call (jolt_host_dory_verify_batch): commitments (n, 48) the tier-2 commitments in claim order, evaluations
    (n, 4) as the statement holds them, point the grid-order point, proof a dict(gts, g1s, g2s) as dory_prove_batch returns, transcript a HostTranscript.
    -> dict(accepted, failed_check, joint_eval)"""
    cm, ev, pt = _gt_rows(commitments), fr(evaluations).reshape(-1, 4), fr(point).reshape(-1, 4)
    if cm.shape[0] != ev.shape[0]:
        raise ValueError("one evaluation per commitment")
    sigma = (pt.shape[0] + 1) // 2
    n_gt, n_g1, n_g2, _ = host_dory_proof_counts(sigma)
    gts, g1s, g2s = _gt_rows(proof["gts"]), _pair_g1(proof["g1s"]), _dory_pts("g2", proof["g2s"])
    if (gts.shape[0], g1s.shape[0], g2s.shape[0]) != (n_gt, n_g1, n_g2):
        raise ValueError("the proof does not have the element counts of an opening of 2^sigma columns")
    accepted, failed, joint = C.c_int32(-1), C.c_int32(-1), fr_array(1)
    _call("jolt_host_dory_verify_batch", self, self.h, verifier.h, verifier.setup.h, _p(cm) if cm.shape[0] else None, _p(ev) if ev.shape[0] else None, cm.shape[0],
          _p(pt), pt.shape[0], _p(gts), _p(g1s), _p(g2s), transcript.h, C.byref(accepted), C.byref(failed), _p(joint))
    return dict(accepted=bool(accepted.value), failed_check=failed.value, joint_eval=joint[0])


Context.dory_gt_pow_many = _dory_gt_pow_many
Context.dory_gt_multi_exp = _dory_gt_multi_exp
Context.dory_verify = _dory_verify
Context.dory_verify_batch = _dory_verify_batch


# ---- HyperKZG verification (hyperkzg_verify.hip): the verifier's setup, its scalars, the verifier as one call, stage 8's batch framing
class HyperKzgVerifierSetup:
    """jolt_hyperkzg_verifier_setup: g1, g2, beta g2 with the line table of (g2, beta g2) resident.  Given `beta` (4 words) the G2 side of setup_from_secret,
    given `beta_g2` (24 words) the three points as a deployment's setup holds them."""

    def __init__(self, ctx, g1, g2, beta=None, beta_g2=None):
        if (beta is None) == (beta_g2 is None):
            raise ValueError("a verifier setup is made from beta or from beta g2")
        self.ctx, self.h = ctx, C.c_void_p()
        p1, p2 = _pair_g1(g1).reshape(12), _dory_pts("g2", g2).reshape(24)
        if beta is not None:
            _call("jolt_hyperkzg_verifier_setup_from_secret", ctx, ctx.h, _p(fr(beta).reshape(4)), _p(p1), _p(p2), C.byref(self.h))
        else:
            _call("jolt_hyperkzg_verifier_setup_create", ctx, ctx.h, _p(p1), _p(p2), _p(_dory_pts("g2", beta_g2).reshape(24)), C.byref(self.h))

    def points(self):
        """(g1 (12,), g2 (24,), beta_g2 (24,)) as the object holds them"""
        g1, g2, bg2 = g1_array(1), g2_array(1), g2_array(1)
        _call("jolt_hyperkzg_verifier_setup_points", self.ctx, self.h, _p(g1), _p(g2), _p(bg2))
        return g1[0], g2[0], bg2[0]

    def close(self):
        if self.h:
            _call("jolt_hyperkzg_verifier_setup_free", self.ctx, self.ctx.h, self.h)
            self.h = None

    free = close


def host_hyperkzg_verify_scalars(point, eval_, v, r, q, d0):
    """jolt_host_hyperkzg_verify_scalars: dict(folding_ok, failed_level, l_scalars (ell + 4, 4), d (2, 4)); v is (3, ell, 4) or (3 ell, 4)"""
    pt, vv = fr(point).reshape(-1, 4), fr(v).reshape(-1, 4)
    ell = pt.shape[0]
    if vv.shape[0] != 3 * ell:
        raise ValueError("v holds 3 ell values")
    ok, level, ls, d = C.c_int32(-1), C.c_size_t(0), fr_array(ell + 4), fr_array(2)
    _call("jolt_host_hyperkzg_verify_scalars", None, ell, _p(pt) if ell else None, _p(fr(eval_).reshape(4)), _p(vv) if ell else None,
          *[_p(fr(x).reshape(4)) for x in (r, q, d0)], C.byref(ok), C.byref(level), _p(ls), _p(d))
    return dict(folding_ok=bool(ok.value), failed_level=level.value, l_scalars=ls, d=d)


def _hyperkzg_proof_in(ell, proof):
    com = np.ascontiguousarray(proof["com"], dtype=np.uint64).reshape(-1, 12)
    w, v = np.ascontiguousarray(proof["w"], dtype=np.uint64).reshape(-1, 12), fr(proof["v"]).reshape(-1, 4)
    if (com.shape[0], w.shape[0], v.shape[0]) != (max(ell, 1) - 1, 3, 3 * ell):
        raise ValueError("the proof does not have the element counts of an opening of ell variables")
    return com, w, v


def _hyperkzg_verify(self, verifier, commitments, point, eval_, proof, transcript=None, callback=None, commitment_scalars=None):
    """HyperKZGScheme::verify as one call (jolt_host_hyperkzg_verify under a HostTranscript, jolt_host_hyperkzg_verify_with_transcript under a callback
    (phase, points (n, 12), values (n, 4)) -> challenge (4,) or a non-zero status).  verifier a HyperKzgVerifierSetup; commitments (12,) or (n, 12) with
    commitment_scalars (n, 4) (None: one commitment under scalar one); proof a dict(com, w, v) as hyperkzg_open returns.
    -> dict(accepted, failed_check, failed_level): failed_check 0 none, 1 the folding check (failed_level names the level), 2 the pairing check.
    A rejected proof raises nothing."""
    if (transcript is None) == (callback is None):
        raise ValueError("a verification runs under a transcript or under a callback")
    cm, pt = np.ascontiguousarray(commitments, dtype=np.uint64).reshape(-1, 12), fr(point).reshape(-1, 4)
    sc = host_fr_from_u64(1).reshape(1, 4) if commitment_scalars is None else fr(commitment_scalars).reshape(-1, 4)
    if cm.shape[0] != sc.shape[0]:
        raise ValueError("one scalar per commitment")
    ell = pt.shape[0]
    com, w, v = _hyperkzg_proof_in(ell, proof)
    accepted, failed, level = C.c_int32(-1), C.c_int32(-1), C.c_size_t(0)
    head = (self.h, verifier.h, _p(cm), _p(sc), cm.shape[0], _p(pt) if ell else None, ell, _p(fr(eval_).reshape(4)), _p(com) if com.shape[0] else None, _p(w),
            _p(v) if ell else None)
    if transcript is not None:
        _call("jolt_host_hyperkzg_verify", self, *head, transcript.h, C.byref(accepted), C.byref(failed), C.byref(level))
    else:
        fn, err = open_transcript_callback(callback)
        st = lib().jolt_host_hyperkzg_verify_with_transcript(*head, fn, None, C.byref(accepted), C.byref(failed), C.byref(level))
        if err:
            raise err[0]
        _ck(st, "jolt_host_hyperkzg_verify_with_transcript", self)
    return dict(accepted=bool(accepted.value), failed_check=failed.value, failed_level=level.value)


def _hyperkzg_prove_batch(self, srs, sources, dense, log_k, evaluations, point, transcript, hint=None, levels=0):
    """HomomorphicBatch::<HyperKZGScheme>::prove_batch as one call (jolt_host_hyperkzg_prove_batch): evaluations (n, 4), one per column in grid_evaluate_columns' order;
    point: log_k + log T coordinates; hint a GridHint over the same sources (None with levels = 0: every level by MSM); transcript a HostTranscript.
    -> dict(com, w, v, challenges, joint_eval)"""
    ev, pt = fr(evaluations).reshape(-1, 4), fr(point).reshape(-1, 4)
    ell = pt.shape[0]
    com, w, v, ch, joint = g1_array(max(ell - 1, 1)), g1_array(3), fr_array(3 * max(ell, 1)), fr_array(3), fr_array(1)
    ss = (C.c_void_p * max(len(sources), 1))(*[s.h for s in sources])
    ds = (C.c_void_p * max(len(dense), 1))(*[t.h for t in dense])
    _call("jolt_host_hyperkzg_prove_batch", self, self.h, srs.h, ss if sources else None, len(sources), ds if dense else None, len(dense), log_k,
          _p(ev) if ev.shape[0] else None, ev.shape[0], _p(pt) if ell else None, ell, hint.h if hint is not None else None, levels, transcript.h, _p(com), _p(w), _p(v), _p(ch),
          _p(joint))
    return dict(com=com[: ell - 1], w=w, v=v.reshape(3, ell, 4), challenges=ch, joint_eval=joint[0])


def _hyperkzg_verify_batch(self, verifier, commitments, evaluations, point, proof, transcript):
    """HomomorphicBatch::<HyperKZGScheme>::verify_batch as one call (jolt_host_hyperkzg_verify_batch): commitments (n, 12) in claim order, evaluations (n, 4).  The
    closing claim is absorbed only after an accepted proof.  -> dict(accepted, failed_check, failed_level, joint_eval)"""
    cm, ev, pt = np.ascontiguousarray(commitments, dtype=np.uint64).reshape(-1, 12), fr(evaluations).reshape(-1, 4), fr(point).reshape(-1, 4)
    if cm.shape[0] != ev.shape[0]:
        raise ValueError("one evaluation per commitment")
    ell = pt.shape[0]
    com, w, v = _hyperkzg_proof_in(ell, proof)
    accepted, failed, level, joint = C.c_int32(-1), C.c_int32(-1), C.c_size_t(0), fr_array(1)
    _call("jolt_host_hyperkzg_verify_batch", self, self.h, verifier.h, _p(cm) if cm.shape[0] else None, _p(ev) if ev.shape[0] else None, cm.shape[0],
          _p(pt) if ell else None, ell, _p(com) if com.shape[0] else None, _p(w), _p(v) if ell else None, transcript.h, C.byref(accepted), C.byref(failed), C.byref(level),
          _p(joint))
    return dict(accepted=bool(accepted.value), failed_check=failed.value, failed_level=level.value, joint_eval=joint[0])


Context.hyperkzg_verifier_setup = lambda self, g1, g2, beta=None, beta_g2=None: HyperKzgVerifierSetup(self, g1, g2, beta=beta, beta_g2=beta_g2)
Context.hyperkzg_verify = _hyperkzg_verify
Context.hyperkzg_prove_batch = _hyperkzg_prove_batch
Context.hyperkzg_verify_batch = _hyperkzg_verify_batch


# ---- the witness commitment in front of an opening (dory.hip, dory_hints.hip.h): row commitments written on the device, normalised, in hint order
def _dory_hints_onehot(self, srs, source, out, chunk_width, first_poly=0, n_polys=None, out_first=0, batch_points=0):
    """the hints of columns [first_poly, first_poly + n_polys) of a OneHot into the G1 vector `out` from element out_first on (jolt_dory_hints_onehot):
    out[out_first + p * k * chunks + row * chunks + chunk]; enqueued, not awaited.  The number of elements written."""
    n_polys = source.n_polys - first_poly if n_polys is None else n_polys
    _call("jolt_dory_hints_onehot", self, self.h, srs.h, source.h, first_poly, n_polys, chunk_width, out.h, out_first, batch_points)
    return n_polys * source.k * (source.cycles // chunk_width)


def _dory_hints_rows(self, srs, values, row_width, out, out_first=0):
    """the row commitments of dory_commit_rows into the G1 vector `out` from element out_first on, normalised (jolt_dory_hints_rows).  The number of rows."""
    _call("jolt_dory_hints_rows", self, self.h, srs.h, values.h, row_width, out.h, out_first)
    return values.count // row_width


def host_dory_g1_normalise(points, run):
    """the per-lane routine of the hint kernel on the host: every point as (x / z^2, y / z^3, 1), the identity as (1, 1, 0), one inversion per `run` points"""
    pts = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 12)
    out = g1_array(max(pts.shape[0], 1))
    _call("jolt_host_dory_g1_normalise", None, _p(pts) if pts.shape[0] else None, pts.shape[0], run, _p(out))
    return out[:pts.shape[0]]


def host_dory_hint_map(k, chunks, window0, e):
    """the hint kernel's index map for one-hot columns: (workspace bucket, hint element) of element e of a launch set that starts at window0"""
    src, dst = C.c_size_t(), C.c_size_t()
    _call("jolt_host_dory_hint_map", None, k, chunks, window0, e, C.byref(src), C.byref(dst))
    return src.value, dst.value


Context.dory_hints_onehot = _dory_hints_onehot
Context.dory_hints_rows = _dory_hints_rows


# ---- the same in the address-major trace placement (dory_am.hip.h): grid index (t << log_block) + (k << log_stride), row r = the cycles [r C, (r + 1) C)
def _dory_hints_onehot_am(self, srs, source, out, sigma, log_block, log_stride=0, first_poly=0, n_polys=None, out_first=0):
    """the address-major hints of columns [first_poly, first_poly + n_polys) of a OneHot into the G1 vector `out` (jolt_dory_hints_onehot_am):
    out[out_first + p * rows + r], rows = cycles >> (sigma - log_block); enqueued, not awaited.  The number of elements written."""
    n_polys = source.n_polys - first_poly if n_polys is None else n_polys
    _call("jolt_dory_hints_onehot_am", self, self.h, srs.h, source.h, first_poly, n_polys, sigma, log_block, log_stride, out.h, out_first)
    return n_polys * (source.cycles >> (sigma - log_block))


def _dory_hints_rows_am(self, srs, values, sigma, log_block, out, out_first=0):
    """the address-major row commitments of a dense column, out[out_first + r] = sum_j values[r C + j] * srs[j << log_block], normalised (jolt_dory_hints_rows_am)"""
    _call("jolt_dory_hints_rows_am", self, self.h, srs.h, values.h, sigma, log_block, out.h, out_first)
    return values.count >> (sigma - log_block)


def _dory_fold_rows_grid_am(self, sources, onehot_scalars, dense, dense_scalars, log_block, log_stride, sigma, left):
    """RlcSource::fold_rows(left, sigma) of the batch's joint polynomial in the address-major placement (jolt_dory_fold_rows_grid_am): 2^sigma entries."""
    hs = (C.c_void_p * max(len(sources), 1))(*[s.h for s in sources])
    ds = (C.c_void_p * max(len(dense), 1))(*[t.h for t in dense])
    osc = fr(np.stack([fr(c) for c in onehot_scalars])).reshape(-1, 4) if len(onehot_scalars) else None
    dsc = fr(np.stack([fr(c) for c in dense_scalars])).reshape(-1, 4) if len(dense_scalars) else None
    h = C.c_void_p()
    _call("jolt_dory_fold_rows_grid_am", self, self.h, hs if sources else None, len(sources), _p(osc), ds if dense else None, len(dense), _p(dsc), log_block, log_stride,
          sigma, left.h, C.byref(h))
    return Table(self, h)


def host_dory_am_place(log_block, log_stride, sigma, cycle, address):
    """(row, column) of the coefficient of (cycle, address) in the address-major matrix of 2^sigma columns"""
    row, col = C.c_size_t(), C.c_size_t()
    _call("jolt_host_dory_am_place", None, log_block, log_stride, sigma, cycle, address, C.byref(row), C.byref(col))
    return row.value, col.value


def host_dory_am_row(bases, hot, k, log_block, log_stride=0):
    """one row of dory_hints_onehot_am through the kernel's accumulation routine and the normalisation: bases (n, 12) with z = 1, hot = the row's hot addresses
    (0xFFFF = cold); the (12,) point"""
    pts = np.ascontiguousarray(bases, dtype=np.uint64).reshape(-1, 12)
    idx = np.ascontiguousarray(hot, dtype=np.uint16)
    out = g1_array(1)
    _call("jolt_host_dory_am_row", None, _p(pts), pts.shape[0], idx.ctypes.data_as(C.c_void_p) if idx.size else None, idx.size, k, log_block, log_stride, _p(out))
    return out[0]


Context.dory_hints_onehot_am = _dory_hints_onehot_am
Context.dory_hints_rows_am = _dory_hints_rows_am
Context.dory_fold_rows_grid_am = _dory_fold_rows_grid_am


# ---- Dory for polynomials held as field elements (dory.hip, dory_rows_fr.hip.h): row commitments of a device table, the block-embedded row fold
DORY_BLOCK_FOLD_SLICE = 64  # kBlockFoldSlice of dory.hip: matrix rows per thread of the block fold


def _dory_commit_rows_fr(self, srs, table, row_width, first=0, count=None):
    """StreamingCommitment::feed(&[Fr]) over every row_width window of table[first, first + count): one G1 point per row (jolt_dory_commit_rows_fr)"""
    count = len(table) - first if count is None else count
    rows = count // row_width if row_width else 0
    out = g1_array(max(rows, 1))
    _call("jolt_dory_commit_rows_fr", self, self.h, srs.h, table.h, first, count, row_width, _p(out))
    return out[:rows]


def _dory_hints_rows_fr(self, srs, table, row_width, out, out_first=0, first=0, count=None):
    """the same rows, normalised, into the G1 vector `out` from element out_first on (jolt_dory_hints_rows_fr).  The number of rows."""
    count = len(table) - first if count is None else count
    _call("jolt_dory_hints_rows_fr", self, self.h, srs.h, table.h, first, count, row_width, out.h, out_first)
    return count // row_width


def _dory_fold_rows_blocks(self, tables, sigma_tables, scalars, sigma, left, base=None):
    """BlockOpeningPoly::fold_rows: out[c] = base[c] + sum_d scalars[d] * sum_r left[r] * tables[d][(r << sigma_tables[d]) + c], every table embedded top-left in
    the grid of 2^sigma columns (jolt_dory_fold_rows_blocks); base: a Table of 2^sigma entries or None.  A Table of 2^sigma entries."""
    n = len(tables)
    if len(sigma_tables) != n or len(scalars) != n:
        raise ValueError("one sigma and one scalar per table")
    hs = (C.c_void_p * max(n, 1))(*[t.h for t in tables])
    sg = (C.c_uint32 * max(n, 1))(*sigma_tables)
    sc = fr(np.stack([fr(c) for c in scalars])).reshape(-1, 4) if n else fr_array(1)
    h = C.c_void_p()
    _call("jolt_dory_fold_rows_blocks", self, self.h, hs, sg, n, _p(sc), sigma, left.h, base.h if base is not None else None, C.byref(h))
    return Table(self, h)


def _dory_fold_rows_blocks_many(self, tables, sigma_tables, scalars, sigma, left, base=None):
    """dory_fold_rows_blocks over up to 256 tables (jolt_dory_fold_rows_blocks_many): a chain of launch sets of eight; the same field elements for any grouping"""
    n = len(tables)
    if len(sigma_tables) != n or len(scalars) != n:
        raise ValueError("one sigma and one scalar per table")
    hs = (C.c_void_p * max(n, 1))(*[t.h for t in tables])
    sg = (C.c_uint32 * max(n, 1))(*sigma_tables)
    sc = fr(np.stack([fr(c) for c in scalars])).reshape(-1, 4) if n else fr_array(1)
    h = C.c_void_p()
    _call("jolt_dory_fold_rows_blocks_many", self, self.h, hs, sg, n, _p(sc), sigma, left.h, base.h if base is not None else None, C.byref(h))
    return Table(self, h)


def _dory_evaluate_blocks(self, tables, sigma_tables, point, sigma):
    """the statement's claims of block-embedded tables from one pass (jolt_dory_evaluate_blocks): (len(tables), 4),
    claims[d] = sum_i tables[d][i] * eq(point, host_dory_block_index(sigma_tables[d], sigma, i)); point: the grid-order opening point of nu + sigma coordinates"""
    n = len(tables)
    if len(sigma_tables) != n:
        raise ValueError("one sigma per table")
    pt = fr(point).reshape(-1, 4)
    if pt.shape[0] < sigma:
        raise ValueError("the point has nu + sigma coordinates")
    hs = (C.c_void_p * max(n, 1))(*[t.h for t in tables])
    sg = (C.c_uint32 * max(n, 1))(*[int(x) for x in sigma_tables])
    out = fr_array(max(n, 1))
    _call("jolt_dory_evaluate_blocks", self, self.h, hs, sg, n, _p(pt) if pt.shape[0] else _p(fr_array(1)), pt.shape[0], pt.shape[0] - sigma, sigma, _p(out))
    return out[:n]


def host_dory_fr_digits(scalar, c, W):
    """the signed c-bit digits the field-row kernels give one scalar: ([digit_w for w < W], negative) with sum_w digit_w 2^(c w) = min(s, r - s) and
    negative = whether r - s was taken"""
    digits, neg = np.zeros(max(W, 1), dtype=np.uint32), C.c_uint32()
    _call("jolt_host_dory_fr_digits", None, _p(fr(scalar)), c, W, _p(digits), C.byref(neg))
    return [-(int(d) & 0x7FFFFFFF) if int(d) >> 31 else int(d) for d in digits[:W]], bool(neg.value)


def host_dory_rows_fr_plan(bit_length, row_width):
    """(c, W) of the field rows for magnitudes of bit_length bits in rows of row_width values"""
    c, W = C.c_int32(), C.c_int32()
    _call("jolt_host_dory_rows_fr_plan", None, bit_length, row_width, C.byref(c), C.byref(W))
    return c.value, W.value


def host_dory_block_index(sigma_table, sigma_grid, i):
    """grid index of coefficient i of a block of 2^sigma_table columns embedded top-left in a grid of 2^sigma_grid columns"""
    out = C.c_size_t()
    _call("jolt_host_dory_block_index", None, sigma_table, sigma_grid, i, C.byref(out))
    return out.value


Context.dory_commit_rows_fr = _dory_commit_rows_fr
Context.dory_hints_rows_fr = _dory_hints_rows_fr
Context.dory_fold_rows_blocks = _dory_fold_rows_blocks
Context.dory_fold_rows_blocks_many = _dory_fold_rows_blocks_many
Context.dory_evaluate_blocks = _dory_evaluate_blocks


def _gt(a):
    return np.ascontiguousarray(a, dtype=np.uint64).reshape(48)


def host_fq12_op(op, a, b=None):
    """Fq12 on the host as the kernels compute it; raises JoltError(1) for an operand that is not canonical, JoltError(11) for the inverse of zero"""
    out = gt_array()
    _call("jolt_host_fq12_op", None, op, _p(_gt(a)), _p(_gt(b)) if b is not None else None, _p(out))
    return out


def host_g2_prepare_one(g2):
    """-> ((PAIRING_LINES, 3, 8) uint64 line coefficients (a, b, c), skip)"""
    lines, skip = np.zeros((PAIRING_LINES, 3, 8), dtype=np.uint64), C.c_int32()
    _call("jolt_host_g2_prepare_one", None, _p(np.ascontiguousarray(g2, dtype=np.uint64).reshape(24)), _p(lines), C.byref(skip))
    return lines, bool(skip.value)


def host_miller_loop(g1s, g2s):
    """the product of the Miller values of the pairs, before the final exponentiation"""
    a, b = _pair_g1(g1s), _dory_pts("g2", g2s)
    if a.shape[0] != b.shape[0]:
        raise ValueError("miller_loop: the two sides differ in length")
    n, out = a.shape[0], gt_array()
    _call("jolt_host_miller_loop", None, _p(a) if n else None, _p(b) if n else None, n, _p(out))
    return out


def host_final_exponentiation(f):
    out = gt_array()
    _call("jolt_host_final_exponentiation", None, _p(_gt(f)), _p(out))
    return out


def host_gt_pow(gt, scalar):
    out = gt_array()
    _call("jolt_host_gt_pow", None, _p(_gt(gt)), _p(fr(scalar)), _p(out))
    return out


def host_hyperkzg_witness_triple(c, g0, g1, r, a, alpha):
    """the three witness commitments of an opening (at r, -r, r^2) from c[k] = commit(X^k Q3), the first two SRS points and the remainders a, alpha, on the host"""
    cs = np.ascontiguousarray(c, dtype=np.uint64).reshape(3, 12)
    p0, p1 = (np.ascontiguousarray(p, dtype=np.uint64).reshape(12) for p in (g0, g1))
    out = g1_array(3)
    _call("jolt_host_hyperkzg_witness_triple", None, _p(cs), _p(p0), _p(p1), _p(fr(r)), _p(fr(a)), _p(fr(alpha)), _p(out))
    return out


Context.dory_fold_rows_grid = _dory_fold_rows_grid
Context.dory_combine_hints = _dory_combine_hints


def _table_op2(name):
    def f(self, a, b):
        h = C.c_void_p()
        _call(name, self, self.h, a.h, b.h, C.byref(h))
        return Table(self, h)
    return f


def _tile(self, base, copies):
    h = C.c_void_p()
    _call("jolt_tile", self, self.h, base.h, copies, C.byref(h))
    return Table(self, h)


def _replicate_stream_lsb(self, base):
    h = C.c_void_p()
    _call("jolt_replicate_stream_lsb", self, self.h, base.h, C.byref(h))
    return Table(self, h)


def _rlc(self, tables, scalars):
    hs = (C.c_void_p * len(tables))(*[t.h for t in tables])
    sc = fr(scalars).reshape(-1, 4)
    h = C.c_void_p()
    _call("jolt_rlc", self, self.h, hs, len(tables), _p(sc), C.byref(h))
    return Table(self, h)


Context.address_fold = _table_op2("jolt_address_fold")
Context.cycle_fold = _table_op2("jolt_cycle_fold")
Context.tile = _tile
Context.replicate_stream_lsb = _replicate_stream_lsb
Context.rlc = _rlc


# ---- device-resident integer promotion, commitment-grid pieces (pcs.hip), memory pool
def _table_from_ints(self, values, offset=0, length=None):
    """Ring::from_u64 / from_i64 / from_i128 of entries [offset, offset+length) of an Ints (already in HBM) as a field table."""
    length = values.count - offset if length is None else length
    h = C.c_void_p()
    _call("jolt_table_from_ints", self, self.h, values.h, offset, length, C.byref(h))
    return Table(self, h)


def _grid_commit_onehot(self, srs, source):
    """KZG commitments of the one-hot columns of `source` over the K x T commitment grid (index k*T + j): (n_polys, 12)."""
    out = g1_array(source.n_polys)
    _call("jolt_grid_commit_onehot", self, self.h, srs.h, source.h, _p(out))
    return out


def _grid_commit_onehot_classes(self, srs, source, shift):
    """(2^shift, n_polys, 12): per residue class c of the cycle mod 2^shift the sums of the bases at (hot * T + j) >> shift (jolt_grid_commit_onehot_classes)"""
    out = g1_array(source.n_polys << shift)
    _call("jolt_grid_commit_onehot_classes", self, self.h, srs.h, source.h, shift, _p(out))
    return out.reshape(1 << shift, source.n_polys, 12)


def _grid_joint_polynomial(self, sources, onehot_scalars, dense, dense_scalars, log_k):
    """Joint polynomial of the stage-8 batch opening over the 2^log_k x T grid (HomomorphicBatch::prove_batch's RLC)."""
    hs = (C.c_void_p * max(len(sources), 1))(*[s.h for s in sources])
    ds = (C.c_void_p * max(len(dense), 1))(*[t.h for t in dense])
    osc = fr(np.stack([fr(c) for c in onehot_scalars])).reshape(-1, 4) if len(onehot_scalars) else None
    dsc = fr(np.stack([fr(c) for c in dense_scalars])).reshape(-1, 4) if len(dense_scalars) else None
    h = C.c_void_p()
    _call("jolt_grid_joint_polynomial", self, self.h, hs if sources else None, len(sources), _p(osc), ds if dense else None, len(dense), _p(dsc), log_k, C.byref(h))
    return Table(self, h)


def _grid_joint_polynomial_subtree(self, sources, onehot_scalars, dense, dense_scalars, log_k, rank, world):
    """The rank's compact array (subtree assignment) of the same joint polynomial: 2^log_k * T / world coefficients."""
    hs = (C.c_void_p * max(len(sources), 1))(*[s.h for s in sources])
    ds = (C.c_void_p * max(len(dense), 1))(*[t.h for t in dense])
    osc = fr(np.stack([fr(c) for c in onehot_scalars])).reshape(-1, 4) if len(onehot_scalars) else None
    dsc = fr(np.stack([fr(c) for c in dense_scalars])).reshape(-1, 4) if len(dense_scalars) else None
    h = C.c_void_p()
    _call("jolt_grid_joint_polynomial_subtree", self, self.h, hs if sources else None, len(sources), _p(osc), ds if dense else None, len(dense), _p(dsc), log_k, rank, world,
          C.byref(h))
    return Table(self, h)


def _trim(self):
    _call("jolt_ctx_trim", self, self.h)


def _memory_stats(self):
    a, b, c = C.c_size_t(), C.c_size_t(), C.c_size_t()
    _call("jolt_ctx_memory_stats", self, self.h, C.byref(a), C.byref(b), C.byref(c))
    out = {"live_bytes": a.value, "cached_bytes": b.value, "peak_bytes": c.value}
    la, ba = C.c_size_t(), C.c_size_t()
    _call("jolt_ctx_workspace_stats", self, self.h, C.byref(la), C.byref(ba))
    out["msm_lanes_bytes"], out["msm_batch_bytes"] = la.value, ba.value  # outside the pool: grow-only MSM workspaces
    gp = C.c_size_t()
    _call("jolt_ctx_grid_pairs_stats", self, self.h, C.byref(gp))
    out["grid_pairs_bytes"] = gp.value  # outside the pool: the commitment grid's pair tables on this context's SRSs
    return out




def _round_path_stats(self, reset=False):
    """Launch counts of the batch rounds per kernel path since the last reset (jolt_ctx_round_path_stats): `group` is keyed by (order, skip_one, fused),
    `split_eq_product` and `bind` are (unfused, fused) and (LowToHigh, HighToLow)."""
    a = np.zeros(ROUND_PATH_COUNT, dtype=np.uint64)
    _call("jolt_ctx_round_path_stats", self, self.h, _p(a), ROUND_PATH_COUNT, 1 if reset else 0)
    c = [int(x) for x in a]
    return {"tail": c[0], "group": {(o, bool(s), bool(f)): c[1 + 4 * o + 2 * s + f] for o in (0, 1) for s in (0, 1) for f in (0, 1)}, "small": c[9],
            "split_eq_product": (c[10], c[11]), "uniform_items": c[12], "uniform_rows": c[13], "lazy": c[14], "bind": (c[15], c[16])}


Context.round_path_stats = _round_path_stats
Context.table_from_ints = _table_from_ints
Context.grid_commit_onehot = _grid_commit_onehot
Context.grid_commit_onehot_classes = _grid_commit_onehot_classes
Context.grid_joint_polynomial = _grid_joint_polynomial
Context.grid_joint_polynomial_subtree = _grid_joint_polynomial_subtree
Context.trim = _trim
Context.memory_stats = _memory_stats


class RwMatrix:
    """Device twin of the optimized RAM read/write-checking kernel's sparse matrix (jolt_rw_matrix_*): same interface as the oracle's
    RwMatrix wrapper plus the fused prove_round."""

    def __init__(self, ctx, addresses, pre, post, inc, val_init, tau_low, gamma):
        """addresses / pre / post: host uint64 arrays (uploaded here), or three u64 Ints already resident in HBM"""
        tau = fr(tau_low).reshape(-1, 4)
        self.ctx = ctx
        h = C.c_void_p()
        if isinstance(addresses, Ints):
            _call("jolt_rw_matrix_create_resident", ctx, ctx.h, addresses.h, pre.h, post.h, inc.h, val_init.h, _p(tau), _p(fr(gamma)), C.byref(h))
        else:
            a, p, q = (np.ascontiguousarray(x, dtype=np.uint64) for x in (addresses, pre, post))
            _call("jolt_rw_matrix_create", ctx, ctx.h, _p(a), _p(p), _p(q), a.shape[0], inc.h, val_init.h, _p(tau), _p(fr(gamma)), C.byref(h))
        self.h = h

    def __len__(self):
        n = C.c_size_t()
        _call("jolt_rw_matrix_len", self.ctx, self.h, C.byref(n))
        return n.value

    def prove_round(self, bind=None):
        evals, aux = fr_array(2), fr_array(3)
        _call("jolt_rw_matrix_prove_round", self.ctx, self.h, _p(fr(bind)) if bind is not None else None, _p(evals), _p(aux))
        return evals, aux

    def finish(self, bind):
        _call("jolt_rw_matrix_finish", self.ctx, self.h, _p(fr(bind)))

    def final_values(self):
        out = fr_array(4)
        _call("jolt_rw_matrix_final_values", self.ctx, self.h, _p(out))
        return out

    def download(self):
        n = len(self)
        rows, cols = np.zeros(max(n, 1), dtype=np.uint64), np.zeros(max(n, 1), dtype=np.uint64)
        val, ra, prev, nxt = fr_array(max(n, 1)), fr_array(max(n, 1)), fr_array(max(n, 1)), fr_array(max(n, 1))
        _call("jolt_rw_matrix_download", self.ctx, self.h, _p(rows), _p(cols), _p(val), _p(ra), _p(prev), _p(nxt))
        return dict(rows=rows[:n], cols=cols[:n], val=val[:n], ra=ra[:n], prev=prev[:n], next=nxt[:n])

    def free(self):
        if self.h:
            lib().jolt_rw_matrix_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


Context.rw_matrix = lambda self, *a, **k: RwMatrix(self, *a, **k)


# ---- the sharded form of both sparse matrices (jolt_rw_matrix_hold_row / _bind / _export_row / _create_merged): shared by RwMatrix and RegistersRw handles
def rw_hold_row(m):
    _call("jolt_rw_matrix_hold_row", m.ctx, m.h)


def rw_bind(m, bind):
    _call("jolt_rw_matrix_bind", m.ctx, m.h, _p(fr(bind)))


def rw_export_row(m, registers):
    """the single row a held local matrix is left with: dict(cols, prev, next (u64), val, ra[, wa] (n, 4), inc, scalar)"""
    n = len(m)
    cap = max(n, 1)
    cols, prev, nxt = (np.zeros(cap, dtype=np.uint64) for _ in range(3))
    val, ra, wa = fr_array(cap), fr_array(cap), fr_array(cap)
    inc, scalar = fr_array(1), fr_array(1)
    got = C.c_size_t()
    _call("jolt_rw_matrix_export_row", m.ctx, m.h, cap, _p(cols), _p(prev), _p(nxt), _p(val), _p(ra), _p(wa) if registers else None, _p(inc), _p(scalar), C.byref(got))
    n = got.value
    out = dict(cols=cols[:n], prev=prev[:n], next=nxt[:n], val=val[:n], ra=ra[:n], inc=inc[0], scalar=scalar[0])
    if registers:
        out["wa"] = wa[:n]
    return out


class MergedRw:
    """jolt_rw_matrix_create_merged: the matrix of the remaining log G cycle variables built from the ranks' exported rows (rank order); continues with the
    ordinary rounds.  registers: the registers flavour (four address-round points, five final values)."""

    def __init__(self, ctx, registers, log_rows, log_k, rows, cols, prev, nxt, val, ra, wa, inc, val_init, w, scalar, gamma):
        self.ctx, self.registers = ctx, bool(registers)
        u = lambda a: np.ascontiguousarray(a, dtype=np.uint64)
        rows, cols, prev, nxt = u(rows), u(cols), u(prev), u(nxt)
        n = rows.shape[0]
        val, ra = u(val).reshape(-1, 4), u(ra).reshape(-1, 4)
        wa = u(wa).reshape(-1, 4) if registers else None
        inc = u(inc).reshape(-1, 4)
        assert inc.shape[0] == 1 << log_rows
        h = C.c_void_p()
        _call("jolt_rw_matrix_create_merged", ctx, ctx.h, 1 if registers else 0, log_rows, log_k, n, _p(rows), _p(cols), _p(prev), _p(nxt), _p(val), _p(ra),
              _p(wa) if registers else None, _p(inc), val_init.h if val_init is not None else None, _p(fr(w).reshape(-1, 4)), _p(fr(scalar)), _p(fr(gamma)), C.byref(h))
        self.h = h

    def __len__(self):
        n = C.c_size_t()
        _call("jolt_rw_matrix_len", self.ctx, self.h, C.byref(n))
        return n.value

    def prove_round(self, bind=None):
        evals, aux = fr_array(4 if self.registers else 2), fr_array(3)
        fn = lib().jolt_registers_rw_prove_round if self.registers else lib().jolt_rw_matrix_prove_round
        _ck(fn(self.h, _p(fr(bind)) if bind is not None else None, _p(evals), _p(aux)), "jolt_rw_matrix_prove_round (merged)", self.ctx)
        return evals, aux

    def finish(self, bind):
        _call("jolt_rw_matrix_finish", self.ctx, self.h, _p(fr(bind)))

    def final_values(self):
        out = fr_array(5 if self.registers else 4)
        fn = lib().jolt_registers_rw_final_values if self.registers else lib().jolt_rw_matrix_final_values
        _ck(fn(self.h, _p(out)), "jolt_rw_matrix_final_values (merged)", self.ctx)
        return out

    def free(self):
        if self.h:
            lib().jolt_rw_matrix_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class KeyIndex:
    """Rows of a resident key column (u64 Ints: bytecode PCs, RAM word addresses; a key >= k is a cold cycle) sorted by key once, for pushforwards
    of cycle weights onto the k-entry address domain (jolt_key_index_*)."""

    def __init__(self, ctx, keys, k):
        self.ctx, self.k = ctx, int(k)
        h = C.c_void_p()
        _call("jolt_key_index_create", ctx, ctx.h, keys.h, self.k, C.byref(h))
        self.h = h

    def size(self):
        cycles, k, items = C.c_size_t(), C.c_uint64(), C.c_uint32()
        _call("jolt_key_index_size", self.ctx, self.h, C.byref(cycles), C.byref(k), C.byref(items))
        return cycles.value, k.value, items.value

    def pushforward(self, weights):
        """weights: list of <= 8 Tables over the cycles -> list of Tables of k entries, out[s][a] = sum of weights[s] over the cycles with key a"""
        n = len(weights)
        hs = (C.c_void_p * n)(*[w.h for w in weights])
        out = (C.c_void_p * n)()
        _call("jolt_key_index_pushforward", self.ctx, self.ctx.h, self.h, hs, n, out)
        return [Table(self.ctx, C.c_void_p(out[i])) for i in range(n)]

    def last_value(self, values, init):
        """values: u64 Ints over the cycles; init: Table of k entries -> Table: the value at the latest cycle of every key, init where a key never occurs"""
        h = C.c_void_p()
        _call("jolt_key_index_last_value", self.ctx, self.ctx.h, self.h, values.h, init.h, C.byref(h))
        return Table(self.ctx, h)

    def free(self):
        if self.h:
            lib().jolt_key_index_destroy(self.ctx.h, self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


Context.key_index = lambda self, keys, k: KeyIndex(self, keys, k)


class RegistersRw:
    """Device twin of the optimized registers read/write-checking kernel (jolt_registers_rw_*): `regs` a OneHot with the columns rs1, rs2, rd,
    the value columns u64 Ints, `inc` the RdInc table."""

    def __init__(self, ctx, regs, rs1_val, rs2_val, rd_pre, rd_post, inc, r_cycle, gamma):
        self.ctx, self.regs = ctx, regs
        h = C.c_void_p()
        _call("jolt_registers_rw_create", ctx, ctx.h, regs.h, rs1_val.h, rs2_val.h, rd_pre.h, rd_post.h, inc.h, _p(fr(r_cycle).reshape(-1, 4)), _p(fr(gamma)), C.byref(h))
        self.h = h

    def __len__(self):
        n = C.c_size_t()
        _call("jolt_rw_matrix_len", self.ctx, self.h, C.byref(n))
        return n.value

    def prove_round(self, bind=None):
        evals, aux = fr_array(4), fr_array(3)
        _call("jolt_registers_rw_prove_round", self.ctx, self.h, _p(fr(bind)) if bind is not None else None, _p(evals), _p(aux))
        return evals, aux

    def finish(self, bind):
        _call("jolt_rw_matrix_finish", self.ctx, self.h, _p(fr(bind)))

    def final_values(self):
        out = fr_array(5)
        _call("jolt_registers_rw_final_values", self.ctx, self.h, _p(out))
        return out

    def download(self):
        n = len(self)
        rows, cols, prev, nxt = (np.zeros(max(n, 1), dtype=np.uint64) for _ in range(4))
        val, ra, wa = fr_array(max(n, 1)), fr_array(max(n, 1)), fr_array(max(n, 1))
        _call("jolt_registers_rw_download", self.ctx, self.h, _p(rows), _p(cols), _p(val), _p(ra), _p(wa), _p(prev), _p(nxt))
        return dict(rows=rows[:n], cols=cols[:n], val=val[:n], ra=ra[:n], wa=wa[:n], prev=prev[:n], next=nxt[:n])

    def free(self):
        if self.h:
            lib().jolt_rw_matrix_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


Context.registers_rw = lambda self, *a, **k: RegistersRw(self, *a, **k)


def _table_dot(self, a, b, deferred=False):
    out = fr_array(1)
    _call("jolt_table_dot", self, self.h, a.h, b.h, 1 if deferred else 0, _p(out))
    return out[0]


Context.table_dot = _table_dot


# ---- Spartan outer T-scale sums (r1cs.hip)
def _handles(tables):
    return (C.c_void_p * max(len(tables), 1))(*[t.h for t in tables])


def _r1cs_uniskip_sums(self, inputs, eq, a_weights, b_weights):
    wa = fr(a_weights).reshape(-1, 2, 1 + len(inputs), 4)
    wb = fr(b_weights).reshape(-1, 2, 1 + len(inputs), 4)
    out = fr_array(wa.shape[0])
    _call("jolt_r1cs_uniskip_sums", self, self.h, _handles(inputs), len(inputs), eq.h, _p(wa), _p(wb), wa.shape[0], _p(out))
    return out


def _r1cs_materialize(self, inputs, a_weights, b_weights):
    wa, wb = fr(a_weights).reshape(2, 1 + len(inputs), 4), fr(b_weights).reshape(2, 1 + len(inputs), 4)
    az, bz = C.c_void_p(), C.c_void_p()
    _call("jolt_r1cs_materialize", self, self.h, _handles(inputs), len(inputs), _p(wa), _p(wb), C.byref(az), C.byref(bz))
    return Table(self, az), Table(self, bz)


def _tables_evaluate(self, tables, point):
    p = fr(point).reshape(-1, 4)
    out = fr_array(len(tables))
    _call("jolt_tables_evaluate", self, self.h, _handles(tables), len(tables), _p(p), p.shape[0], _p(out))
    return out


def _r1cs_uniskip_sums_small(self, inputs, eq, a_weights, b_weights, streams=2):
    """inputs: Ints columns; a_weights / b_weights: int64 [node][stream][1 + n] (integer Lagrange-extension column weights);
    streams = 2: Spartan outer, streams = 1: product virtualization (no stream variable)"""
    wa = np.ascontiguousarray(a_weights, dtype=np.int64).reshape(-1, streams, 1 + len(inputs))
    wb = np.ascontiguousarray(b_weights, dtype=np.int64).reshape(-1, streams, 1 + len(inputs))
    out = fr_array(wa.shape[0])
    _call("jolt_r1cs_uniskip_sums_small", self, self.h, _handles(inputs), len(inputs), eq.h, streams, wa.ctypes.data_as(C.c_void_p), wb.ctypes.data_as(C.c_void_p),
          wa.shape[0], _p(out))
    return out


def _r1cs_materialize_small(self, inputs, a_weights, b_weights, streams=2):
    wa, wb = fr(a_weights).reshape(streams, 1 + len(inputs), 4), fr(b_weights).reshape(streams, 1 + len(inputs), 4)
    az, bz = C.c_void_p(), C.c_void_p()
    _call("jolt_r1cs_materialize_small", self, self.h, _handles(inputs), len(inputs), streams, _p(wa), _p(wb), C.byref(az), C.byref(bz))
    return Table(self, az), Table(self, bz)


def _ints_evaluate(self, columns, point):
    p = fr(point).reshape(-1, 4)
    out = fr_array(len(columns))
    _call("jolt_ints_evaluate", self, self.h, _handles(columns), len(columns), _p(p), p.shape[0], _p(out))
    return out


Context.r1cs_uniskip_sums_small = _r1cs_uniskip_sums_small
Context.r1cs_materialize_small = _r1cs_materialize_small
Context.ints_evaluate = _ints_evaluate
Context.r1cs_uniskip_sums = _r1cs_uniskip_sums
Context.r1cs_materialize = _r1cs_materialize
Context.tables_evaluate = _tables_evaluate


def _rows_window_table(self, offset, width, signed=False, lookahead=0, cycles=None, padding_value=0, none_value=0):
    """RandomAccessRows::window: field of row j (or j + 1) for every cycle of the padded domain, padding / None rows as given."""
    cycles = self.n_rows if cycles is None else cycles
    h = C.c_void_p()
    _call("jolt_table_from_rows_window", self.ctx, self.ctx.h, self.h, offset, width, 1 if signed else 0, lookahead, cycles, padding_value, none_value, C.byref(h))
    return Table(self.ctx, h)


def _rows_onehot_sentinel(self, offset, width, shifts, log_k, cycles=None):
    """hot-index columns from a `value + 1, 0 = none` packed address field (InstructionCycleRow)"""
    cycles = self.n_rows if cycles is None else cycles
    sh = (C.c_uint32 * len(shifts))(*shifts)
    h = C.c_void_p()
    _call("jolt_onehot_from_rows_sentinel", self.ctx, self.ctx.h, self.h, offset, width, sh, len(shifts), log_k, cycles, C.byref(h))
    src = OneHot.__new__(OneHot)
    src.ctx, src.n_polys, src.cycles, src.k, src.h, src.wide = self.ctx, len(shifts), cycles, 1 << log_k, h, log_k > 7
    return src


Rows.window_table = _rows_window_table
Rows.onehot_sentinel = _rows_onehot_sentinel


# ---- instruction read+RAF checking scans (read_raf.hip) ---------------------------------------------------------------------------
class ReadRaf:
    """lookup_index: (T, 2) uint64 (lo, hi); table_index: uint8 (0xFF = none); raf_flag: uint8"""

    def __init__(self, ctx, lookup_index, table_index, raf_flag, n_tables):
        idx = np.ascontiguousarray(lookup_index, dtype=np.uint64).reshape(-1, 2)
        tab = np.ascontiguousarray(table_index, dtype=np.uint8)
        raf = np.ascontiguousarray(raf_flag, dtype=np.uint8)
        assert idx.shape[0] == tab.shape[0] == raf.shape[0]
        self.ctx, self.cycles, self.n_tables = ctx, idx.shape[0], n_tables
        h = C.c_void_p()
        _call("jolt_read_raf_create", ctx, ctx.h, idx.ctypes.data_as(C.c_void_p), tab.ctypes.data_as(C.c_void_p), raf.ctypes.data_as(C.c_void_p), self.cycles, n_tables,
              C.byref(h))
        self.h = h

    def phase_scan(self, u, suffix_len, address_bits, suffix_lists, canonical=False):
        """suffix_lists: per table the list of suffix kind ids -> (raf (6, 256, 4), suffix sums (total, 256, 4))"""
        offs = np.zeros(self.n_tables + 1, dtype=np.uint32)
        offs[1:] = np.cumsum([len(l) for l in suffix_lists])
        kinds = np.array([k for l in suffix_lists for k in l], dtype=np.uint8)
        raf = fr_array(6 * 256)
        suf = fr_array(max(int(offs[-1]) * 256, 1))
        _call("jolt_read_raf_phase_scan", self.ctx, self.ctx.h, self.h, u.h, suffix_len, address_bits, 1 if canonical else 0, offs.ctypes.data_as(C.c_void_p),
              kinds.ctypes.data_as(C.c_void_p) if kinds.size else None, _p(raf), _p(suf))
        return raf.reshape(6, 256, 4), suf[: int(offs[-1]) * 256].reshape(-1, 256, 4)

    def condense(self, u, v_table, shift):
        v = fr(v_table).reshape(256, 4)
        _call("jolt_read_raf_condense", self.ctx, self.ctx.h, self.h, u.h, _p(v), shift)

    def cycle_tables(self, table_values, raf_interleaved, raf_identity, v_tables, address_bits, ra_count):
        tv = fr(table_values).reshape(self.n_tables, 4)
        vt = fr(v_tables).reshape(-1, 256, 4)
        combined = C.c_void_p()
        ra = (C.c_void_p * ra_count)()
        _call("jolt_read_raf_cycle_tables", self.ctx, self.ctx.h, self.h, _p(tv), _p(fr(raf_interleaved).reshape(4)), _p(fr(raf_identity).reshape(4)), _p(vt), vt.shape[0],
              address_bits, ra_count, C.byref(combined), ra)
        return Table(self.ctx, combined), [Table(self.ctx, C.c_void_p(p)) for p in ra]

    def free(self):
        if self.h:
            lib().jolt_read_raf_destroy(self.ctx.h, self.h)
            self.h = None


Context.read_raf = lambda self, lookup_index, table_index, raf_flag, n_tables: ReadRaf(self, lookup_index, table_index, raf_flag, n_tables)


def host_fq_limb_op(op, a, b=None, c=None, d=None):
    """fq_limb.hip.h on the host: op 0 a*b, 1 a^2, 2 a*b + c*d, 3 (a - b)*c, 4 (a - b - 2c)*d over canonical Fq (standard Montgomery limbs)"""
    o = fr_array(1)
    arg = lambda x: _p(fr(x)) if x is not None else None
    _call("jolt_host_fq_limb_op", None, op, arg(a), arg(b), arg(c), arg(d), _p(o))
    return o[0]


def host_g1_sum_limb_form(points, negate=None):
    """sum of affine points ((n, 8) uint64: x, y in standard Montgomery form; (0, 0) = infinity) through the limb-form XYZZ accumulator"""
    pts = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 8)
    neg = np.ascontiguousarray(negate if negate is not None else np.zeros(pts.shape[0]), dtype=np.uint8)
    out = g1_array(1)
    _call("jolt_host_g1_sum_limb_form", None, pts.ctypes.data_as(C.c_void_p), neg.ctypes.data_as(C.c_void_p), pts.shape[0], _p(out))
    return out[0]


def host_g1xl_add_paths(acc, q, negate=False):
    """one limb-form mixed addition through both paths of fq_limb.hip.h.  acc: 36 uint32 limbs (X, Y, ZZ, ZZZ), q: 18 limbs (qx, qy).
    Returns dict(common, full, step: (4, 9) uint32 limbs; suspect: bool; canon_common, canon_full: (4, 8) uint32 standard Montgomery words)"""
    a = np.ascontiguousarray(acc, dtype=np.uint32).reshape(36)
    b = np.ascontiguousarray(q, dtype=np.uint32).reshape(18)
    common, full, step = (np.zeros((4, 9), dtype=np.uint32) for _ in range(3))
    canon = np.zeros((2, 4, 8), dtype=np.uint32)
    sus = C.c_int32()
    vp = lambda x: x.ctypes.data_as(C.c_void_p)
    _call("jolt_host_g1xl_add_paths", None, vp(a), vp(b), 1 if negate else 0, vp(common), vp(full), vp(step), C.byref(sus), vp(canon))
    return {"common": common, "full": full, "step": step, "suspect": bool(sus.value), "canon_common": canon[0], "canon_full": canon[1]}


def host_fx_digits(scalar, window_bits):
    """(signed digits as Python ints, bucket count) of the fixed-base MSM's recoding of one Montgomery-form scalar"""
    keys = np.zeros(64, dtype=np.uint32)
    nw, nb = C.c_uint32(), C.c_uint32()
    _call("jolt_host_fx_digits", None, _p(fr(scalar)), window_bits, keys.ctypes.data_as(C.c_void_p), C.byref(nw), C.byref(nb))
    return [(-1 if int(k) >> 31 else 1) * (int(k) & 0x7FFFFFFF) for k in keys[: nw.value]], nb.value


def host_fx_segment_capacity(n, window_bits, segment):
    """the region (in entries) the capacity sort of an n-term fixed-base MSM gives segment `segment` of 256 buckets (jolt_host_fx_segment_capacity)"""
    cap = C.c_uint32()
    _call("jolt_host_fx_segment_capacity", None, n, window_bits, segment, C.byref(cap))
    return int(cap.value)


def host_suffix_mle(kind, bits, length):
    out = C.c_uint64()
    _call("jolt_host_suffix_mle", None, kind, bits & (2**64 - 1), (bits >> 64) & (2**64 - 1), length, C.byref(out))
    return out.value


def host_small_scalar_dot(values, scalars):
    """sum_k values[k] * scalars[k] (Python ints within i128) through the device's small-scalar accumulator, on the host"""
    v = fr(values).reshape(-1, 4)
    sc = np.array([[int(x) & (2**64 - 1), (int(x) >> 64) & (2**64 - 1)] for x in scalars], dtype=np.uint64).reshape(-1, 2)
    o = fr_array(1)
    _call("jolt_host_small_scalar_dot", None, _p(v), sc.ctypes.data_as(C.c_void_p), v.shape[0], _p(o))
    return o[0]


# ---- instruction read+RAF: the address rounds on the host (read_raf_address.hip, lookup_tables.hpp) ---------------------------------------------------------
NUM_LOOKUP_TABLES, NUM_LOOKUP_PREFIXES = 42, 49


def lookup_table_suffixes(kind):
    out, n = np.zeros(8, dtype=np.uint8), C.c_uint32()
    _call("jolt_lookup_table_suffixes", None, kind, _p(out), C.byref(n))
    return [int(k) for k in out[: n.value]]


def lookup_table_prefixes(kind):
    out, n = np.zeros(8, dtype=np.uint8), C.c_uint32()
    _call("jolt_lookup_table_prefixes", None, kind, _p(out), C.byref(n))
    return [int(k) for k in out[: n.value]]


def lookup_suffix_lists():
    """LookupTableKind::suffixes() of the 42 tables: the suffix_lists argument of ReadRaf.phase_scan for real tables"""
    offs = np.zeros(NUM_LOOKUP_TABLES + 1, dtype=np.uint32)
    _call("jolt_lookup_suffix_layout", None, _p(offs), None)
    kinds = np.zeros(int(offs[-1]), dtype=np.uint8)
    _call("jolt_lookup_suffix_layout", None, _p(offs), _p(kinds))
    return [[int(k) for k in kinds[offs[t]: offs[t + 1]]] for t in range(NUM_LOOKUP_TABLES)]


def host_lookup_prefix_default_checkpoints():
    out = fr_array(NUM_LOOKUP_PREFIXES)
    _call("jolt_host_lookup_prefix_default_checkpoints", None, _p(out))
    return out


def host_lookup_prefix_evaluate(prefix, checkpoints, b, b_len, suffix_len):
    out = fr_array(1)
    _call("jolt_host_lookup_prefix_evaluate", None, prefix, _p(fr(checkpoints).reshape(NUM_LOOKUP_PREFIXES, 4)), b, b_len, suffix_len, _p(out))
    return out[0]


def host_lookup_prefix_table(prefix, checkpoints, b_len, suffix_len):
    out = fr_array(1 << b_len)
    _call("jolt_host_lookup_prefix_table", None, prefix, _p(fr(checkpoints).reshape(NUM_LOOKUP_PREFIXES, 4)), b_len, suffix_len, _p(out))
    return out


def host_lookup_table_combine(kind, prefixes, suffixes):
    out = fr_array(1)
    _call("jolt_host_lookup_table_combine", None, kind, _p(fr(prefixes).reshape(NUM_LOOKUP_PREFIXES, 4)), _p(fr(suffixes).reshape(-1, 4)), _p(out))
    return out[0]


class HostReadRafAddress:
    """The 256-entry state of the 16 address phases (jolt_host_read_raf_address_*): prefix polynomials, suffix accumulators, RAF decompositions, checkpoints"""

    def __init__(self, gamma, table_present, canonical=False):
        present = np.zeros(NUM_LOOKUP_TABLES, dtype=np.uint8)
        present[: len(table_present)] = np.asarray(table_present, dtype=np.uint8)
        h = C.c_void_p()
        _call("jolt_host_read_raf_address_create", None, _p(fr(gamma).reshape(4)), _p(present), 1 if canonical else 0, C.byref(h))
        self.h = h

    def init_phase(self, phase, raf_sums, suffix_sums):
        _call("jolt_host_read_raf_address_init_phase", None, self.h, phase, _p(fr(raf_sums).reshape(6 * 256, 4)), _p(fr(suffix_sums).reshape(-1, 4)))

    def message(self, previous_claim=None):
        """s(0), s(1), s(2); without a running claim s(1) is summed from the tables (round 0: s(0) + s(1) = the input claim)"""
        o = fr_array(3)
        _call("jolt_host_read_raf_address_message", None, self.h, _p(fr(previous_claim).reshape(4)) if previous_claim is not None else None, _p(o))
        return o

    def bind(self, r):
        done = C.c_int32()
        _call("jolt_host_read_raf_address_bind", None, self.h, _p(fr(r).reshape(4)), C.byref(done))
        return bool(done.value)

    def prove_phase(self, claim, transcript):
        """the 8 rounds of the open phase against a HostTranscript: -> (claim after the phase, coefficients (8, 3, 4), challenges (8, 4))"""
        c = fr(claim).reshape(4).copy()
        coeffs, challenges = fr_array(24), fr_array(8)
        _call("jolt_host_read_raf_address_prove_phase", None, self.h, _p(c), None, None, transcript.h, _p(coeffs), _p(challenges))
        return c, coeffs.reshape(8, 3, 4), challenges

    def v_table(self, phase):
        o = fr_array(256)
        _call("jolt_host_read_raf_address_v_table", None, self.h, phase, _p(o))
        return o

    def finish(self):
        tv, a, b = fr_array(NUM_LOOKUP_TABLES), fr_array(1), fr_array(1)
        _call("jolt_host_read_raf_address_finish", None, self.h, _p(tv), _p(a), _p(b))
        return tv, a[0], b[0]

    def close(self):
        if self.h:
            lib().jolt_host_read_raf_address_destroy(self.h)
            self.h = None


def host_small_round_pair(n_tables, groups, is_int, int_pairs, fr_pairs, n_evals, skip_one):
    """jolt_host_small_round_pair: the per-pair evaluation of the integer round kernel (small_round.hip.h) compiled for the host.  groups as in Context.member_lc;
    int_pairs (n_tables, 2) uint64, fr_pairs (n_tables, 2, 4) Montgomery limbs -> (n_evals, 4)"""
    goff, foff, consts, ltab, lcoef = [0], [0], [], [], []
    zero = np.zeros(4, dtype=np.uint64)
    for g in groups:
        for const, entries in g:
            consts.append(zero if const is None else fr(const))
            for c, ti in entries:
                lcoef.append(fr(c))
                ltab.append(ti)
            foff.append(len(ltab))
        goff.append(len(consts))
    goff, foff = np.array(goff, dtype=np.uint32), np.array(foff, dtype=np.uint32)
    consts_a = np.ascontiguousarray(np.stack(consts)) if consts else fr_array(1)
    ltab_a = np.array(ltab if ltab else [0], dtype=np.uint32)
    lcoef_a = np.ascontiguousarray(np.stack(lcoef)) if lcoef else fr_array(1)
    d = MemberLcDesc(n_tables, len(groups), len(consts), len(ltab), n_evals, ORDER_LOW_TO_HIGH, 0, goff.ctypes.data, foff.ctypes.data, consts_a.ctypes.data, ltab_a.ctypes.data,
                     lcoef_a.ctypes.data)
    mask = np.ascontiguousarray(is_int, dtype=np.uint8)
    ip = np.ascontiguousarray(int_pairs, dtype=np.uint64).reshape(n_tables, 2)
    fp = np.ascontiguousarray(fr_pairs, dtype=np.uint64).reshape(n_tables, 2, 4)
    out = fr_array(n_evals)
    _call("jolt_host_small_round_pair", None, C.byref(d), _p(mask), _p(ip), _p(fp), n_evals, 1 if skip_one else 0, _p(out))
    return out


# ---- stage operators as ProveRounds objects (stage_ops.hip): one per backend slot ---------------------------------------------------------------------------
class StageOp:
    """jolt_stage_op: prove_round / finish_rounds / output_claims of one stage operator.  `keep`: Python objects the operator borrows (they must outlive it)."""

    def __init__(self, ctx, handle, keep=()):
        self.ctx, self.h, self._keep = ctx, handle, list(keep)

    @property
    def rounds(self):
        n = C.c_size_t()
        _call("jolt_stage_op_num_rounds", self.ctx, self.h, C.byref(n))
        return n.value

    @property
    def degree(self):
        n = C.c_size_t()
        _call("jolt_stage_op_degree", self.ctx, self.h, C.byref(n))
        return n.value

    def input_claim(self):
        o = fr_array(1)
        _call("jolt_stage_op_input_claim", self.ctx, self.h, _p(o))
        return o[0]

    def prove_round(self, bind, rnd, previous_claim):
        """ProveRounds::prove_round: the round message as coefficients (n, 4)"""
        cap = self.degree + 1
        out, n = fr_array(cap), C.c_size_t()
        _call("jolt_stage_op_prove_round", self.ctx, self.h, _p(fr(bind)) if bind is not None else None, rnd, _p(fr(previous_claim)), _p(out), cap, C.byref(n))
        return out[: n.value].copy()

    def finish_rounds(self, bind):
        _call("jolt_stage_op_finish_rounds", self.ctx, self.h, _p(fr(bind)))

    def output_claims(self):
        n = C.c_size_t()
        out = fr_array(320)  # (a precommitted reduction answers with up to 1 + 256 claims)
        _call("jolt_stage_op_output_claims", self.ctx, self.h, _p(out), 320, C.byref(n))
        return out[: n.value].copy()

    def kept(self, key):
        n = C.c_size_t()
        _call("jolt_stage_op_kept", self.ctx, self.h, key.encode(), None, 0, C.byref(n))
        out = fr_array(max(n.value, 1))
        _call("jolt_stage_op_kept", self.ctx, self.h, key.encode(), _p(out), n.value, C.byref(n))
        return out[: n.value]

    def window(self, first, n):
        h = C.c_void_p()
        _call("jolt_stage_op_window", self.ctx, self.h, first, n, C.byref(h))
        return StageOp(self.ctx, h, keep=[self])

    def prove_alone(self, transcript, claim):
        """jolt_host_stage_op_prove_alone: -> dict(polys = per round the message's coefficients, challenges, final_claim)"""
        rounds, stride = self.rounds, self.degree + 1
        c = fr(claim).reshape(4).copy()
        coeffs, counts, chal = fr_array(max(rounds * stride, 1)), np.zeros(max(rounds, 1), dtype=np.uint32), fr_array(max(rounds, 1))
        _call("jolt_host_stage_op_prove_alone", self.ctx, self.h, transcript.h, _p(c), _p(coeffs), stride, counts.ctypes.data_as(C.c_void_p), _p(chal))
        coeffs = coeffs.reshape(-1, stride, 4)
        return dict(polys=[coeffs[r, : counts[r]].copy() for r in range(rounds)], challenges=chal[:rounds].copy() if rounds else np.zeros((0, 4), dtype=np.uint64), final_claim=c)

    def destroy(self):
        if self.h:
            lib().jolt_stage_op_destroy(self.h)
            self.h = None
        self._keep = []

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


def stage_host_expr(tables, terms, degree):
    """jolt_stage_host_expr_create: the dense member over HOST tables as a stage operator (no device, no context): terms = [(coeff_limbs, [table indices]), ...]"""
    tabs = [np.ascontiguousarray(t, dtype=np.uint64).reshape(-1, 4) for t in tables]
    offs, facs = [0], []
    for _, f in terms:
        facs.extend(f)
        offs.append(len(facs))
    offs = np.array(offs, dtype=np.uint32)
    facs_a = np.array(facs if facs else [0], dtype=np.uint32)
    coeffs = np.ascontiguousarray(np.stack([fr(c) for c, _ in terms])).reshape(-1, 4)
    d = MemberDesc(len(tabs), len(terms), degree, ORDER_LOW_TO_HIGH, offs.ctypes.data, facs_a.ctypes.data, coeffs.ctypes.data)
    ptrs = (C.c_void_p * len(tabs))(*[t.ctypes.data for t in tabs])
    h = C.c_void_p()
    _call("jolt_stage_host_expr_create", None, ptrs, tabs[0].shape[0], C.byref(d), C.byref(h))
    return StageOp(None, h)


def prove_batch_ops(ops, input_claims, coefficients, offsets, max_num_vars, max_degree, label=0, challenge_mode=0):
    """jolt_host_prove_batch_ops without a context (host-only operators)"""
    return _prove_batch_ops(None, ops, input_claims, coefficients, offsets, max_num_vars, max_degree, label, challenge_mode)


def prove_batch_ops_grouped(ops, input_claims, coefficients, offsets, max_num_vars, max_degree, label=0, challenge_mode=0):
    """jolt_host_prove_batch_ops_grouped without a context (host-only operators)"""
    return _prove_batch_ops(None, ops, input_claims, coefficients, offsets, max_num_vars, max_degree, label, challenge_mode, grouped=True)


def _prove_batch_ops(self, ops, input_claims, coefficients, offsets, max_num_vars, max_degree, label=0, challenge_mode=0, grouped=False):
    """prove_batch (prover.rs:193-362) over stage operators (jolt_host_prove_batch_ops): the same outputs as Context.prove_batch.  grouped: jolt_host_prove_batch_ops_grouped --
    the operators that are device members (Context.stage_member) go through one round-group launch set per round; the same bytes"""
    n = len(ops)
    hs = (C.c_void_p * n)(*[o.h for o in ops])
    ic = np.ascontiguousarray(np.stack(input_claims), dtype=np.uint64).reshape(-1, 4)
    co = np.ascontiguousarray(np.stack(coefficients), dtype=np.uint64).reshape(-1, 4)
    offs = (C.c_size_t * n)(*offsets)
    polys, chal = fr_array(max(max_num_vars * (max_degree + 1), 1)), fr_array(max(max_num_vars, 1))
    mclaims, final = fr_array(n), fr_array(1)
    name = "jolt_host_prove_batch_ops_grouped" if grouped else "jolt_host_prove_batch_ops"
    _call(name, self, self.h if self is not None else None, hs, n, _p(ic), _p(co), offs, max_num_vars, max_degree, label, challenge_mode, _p(polys), _p(chal), _p(mclaims),
          _p(final))
    return dict(polys=polys[: max_num_vars * (max_degree + 1)].reshape(max_num_vars, max_degree + 1, 4), challenges=chal[:max_num_vars], member_claims=mclaims, final_claim=final[0])


def _stage_spartan_uniskip_sums(self, cols, tau, a_weights, b_weights, streams):
    wa = np.ascontiguousarray(a_weights, dtype=np.int64).reshape(-1, streams, 1 + len(cols))
    wb = np.ascontiguousarray(b_weights, dtype=np.int64).reshape(-1, streams, 1 + len(cols))
    t = fr(tau).reshape(-1, 4)
    out = fr_array(wa.shape[0])
    _call("jolt_stage_spartan_uniskip_sums", self, self.h, _handles(cols), len(cols), streams, _p(t), t.shape[0], wa.ctypes.data_as(C.c_void_p), wb.ctypes.data_as(C.c_void_p),
          wa.shape[0], _p(out))
    return out


def _stage_spartan_remainder(self, cols, fa, fb, tau, scale, streams):
    wa, wb = fr(fa).reshape(streams, 1 + len(cols), 4), fr(fb).reshape(streams, 1 + len(cols), 4)
    t = fr(tau).reshape(-1, 4)
    h = C.c_void_p()
    _call("jolt_stage_spartan_remainder_create", self, self.h, _handles(cols), len(cols), streams, _p(wa), _p(wb), _p(t), t.shape[0],
          _p(fr(scale)) if scale is not None else None, C.byref(h))
    return StageOp(self, h, keep=cols)


def _stage_ram_read_write(self, addresses, pre, post, inc, val_init, tau_low, gamma):
    h = C.c_void_p()
    _call("jolt_stage_ram_read_write_create", self, self.h, addresses.h, pre.h, post.h, inc.h, val_init.h, _p(fr(tau_low).reshape(-1, 4)), _p(fr(gamma)), C.byref(h))
    return StageOp(self, h, keep=[addresses, pre, post, inc, val_init])


def _stage_registers_read_write(self, regs, rs1_val, rs2_val, rd_pre, rd_post, inc, r_cycle, gamma):
    h = C.c_void_p()
    _call("jolt_stage_registers_read_write_create", self, self.h, regs.h, rs1_val.h, rs2_val.h, rd_pre.h, rd_post.h, inc.h, _p(fr(r_cycle).reshape(-1, 4)), _p(fr(gamma)),
          C.byref(h))
    return StageOp(self, h, keep=[regs, rs1_val, rs2_val, rd_pre, rd_post, inc])


def _stage_booleanity_address(self, cols, reference_cycle, reference_address, gamma):
    rc = fr(reference_cycle).reshape(-1, 4)
    h = C.c_void_p()
    _call("jolt_stage_booleanity_address_create", self, self.h, cols.h, _p(rc), rc.shape[0], _p(fr(reference_address).reshape(-1, 4)), _p(fr(gamma)), C.byref(h))
    return StageOp(self, h, keep=[cols])


def _stage_booleanity_cycle(self, cols, r_address, reference_address, reference_cycle, gamma):
    rc = fr(reference_cycle).reshape(-1, 4)
    h = C.c_void_p()
    _call("jolt_stage_booleanity_cycle_create", self, self.h, cols.h, _p(fr(r_address).reshape(-1, 4)), _p(fr(reference_address).reshape(-1, 4)), _p(rc), rc.shape[0],
          _p(fr(gamma)), C.byref(h))
    return StageOp(self, h, keep=[cols])


def _stage_hamming_weight(self, cols, r_cycle, r_address, virtualization_points, gamma):
    rc = fr(r_cycle).reshape(-1, 4)
    h = C.c_void_p()
    _call("jolt_stage_hamming_weight_create", self, self.h, cols.h, _p(rc), rc.shape[0], _p(fr(r_address).reshape(-1, 4)),
          _p(np.ascontiguousarray(virtualization_points, dtype=np.uint64).reshape(-1, 4)), _p(fr(gamma)), C.byref(h))
    return StageOp(self, h, keep=[cols])


def _stage_instruction_read_raf(self, rows, claim_columns, r_reduction, gamma, table_present, ra_count):
    rr = fr(r_reduction).reshape(-1, 4)
    present = np.zeros(NUM_LOOKUP_TABLES, dtype=np.uint8)
    present[: len(table_present)] = np.asarray(table_present, dtype=np.uint8)
    h = C.c_void_p()
    _call("jolt_stage_instruction_read_raf_create", self, self.h, rows.h, claim_columns.h, _p(rr), rr.shape[0], _p(fr(gamma)), _p(present), ra_count, C.byref(h))
    return StageOp(self, h, keep=[rows, claim_columns])


def _stage_bytecode_read_raf_address(self, pc_index, stage_points, stage_values, gamma, first_pc, entry_index):
    sp = np.ascontiguousarray(stage_points, dtype=np.uint64).reshape(5, -1, 4)
    sv = np.ascontiguousarray(stage_values, dtype=np.uint64).reshape(5, -1, 4)
    h = C.c_void_p()
    _call("jolt_stage_bytecode_read_raf_address_create", self, self.h, pc_index.h, _p(sp), sp.shape[1], _p(sv), _p(fr(gamma)), int(first_pc), int(entry_index), C.byref(h))
    return StageOp(self, h, keep=[pc_index])


def _stage_bytecode_read_raf_cycle(self, address_op, pc_chunks, chunk_bits):
    h = C.c_void_p()
    _call("jolt_stage_bytecode_read_raf_cycle_create", self, self.h, address_op.h, pc_chunks.h, chunk_bits, C.byref(h))
    return StageOp(self, h, keep=[pc_chunks])


def _stage_ram_raf_evaluation(self, ram_index, tau_low, lowest_address):
    t = fr(tau_low).reshape(-1, 4)
    h = C.c_void_p()
    _call("jolt_stage_ram_raf_evaluation_create", self, self.h, ram_index.h, _p(t), t.shape[0], int(lowest_address), C.byref(h))
    return StageOp(self, h, keep=[ram_index])


def _stage_ram_output_check(self, ram_index, post_values, val_init, val_io, io_lo, io_len, r_address):
    vi, vo = np.ascontiguousarray(val_init, dtype=np.uint64), np.ascontiguousarray(val_io, dtype=np.uint64)
    h = C.c_void_p()
    _call("jolt_stage_ram_output_check_create", self, self.h, ram_index.h, post_values.h, _p(vi), _p(vo), int(io_lo), int(io_len), _p(fr(r_address).reshape(-1, 4)),
          C.byref(h))
    return StageOp(self, h, keep=[ram_index, post_values])




def _stage_member(self, member, own=False):
    """jolt_stage_member_create: a device Member as a stage operator.  It borrows `member` (which stays the caller's: reset() after the operator is destroyed makes it
    provable again) unless own=True, in which case destroying the operator destroys the member and the Member handle is emptied here."""
    h = C.c_void_p()
    _call("jolt_stage_member_create", self, self.h, member.h if member is not None else None, STAGE_MEMBER_OWN if own else 0, C.byref(h))
    if own:
        member.h = None
    return StageOp(self, h, keep=[member])


Context.stage_member = _stage_member
Context.prove_batch_ops = _prove_batch_ops
Context.prove_batch_ops_grouped = lambda self, *a, **k: _prove_batch_ops(self, *a, grouped=True, **k)
Context.stage_spartan_uniskip_sums = _stage_spartan_uniskip_sums
Context.stage_spartan_remainder = _stage_spartan_remainder
Context.stage_ram_read_write = _stage_ram_read_write
Context.stage_registers_read_write = _stage_registers_read_write
Context.stage_booleanity_address = _stage_booleanity_address
Context.stage_booleanity_cycle = _stage_booleanity_cycle
Context.stage_hamming_weight = _stage_hamming_weight
Context.stage_instruction_read_raf = _stage_instruction_read_raf
Context.stage_bytecode_read_raf_address = _stage_bytecode_read_raf_address
Context.stage_bytecode_read_raf_cycle = _stage_bytecode_read_raf_cycle
Context.stage_ram_raf_evaluation = _stage_ram_raf_evaluation
Context.stage_ram_output_check = _stage_ram_output_check


# ---- a constraint system as rows, the uni-skip round above it (r1cs_rows.hip, small_r1cs.hip, stage_ops.hip) ---------------------------------------------------
class R1csRows:
    """jolt_r1cs_rows: streams = per stream a list of rows (a_terms, a_const, b_terms, b_const) at the domain positions 0, 1, ...; terms = [(input index, int64 coefficient)],
    b_const any integer of 128 signed bits.  No device, no context."""

    def __init__(self, streams, domain_size, n_inputs, zero_on_domain=True):
        rows = [r for st in streams for r in st]
        def flat(side):
            offs, cols, cfs = [0], [], []
            for r in rows:
                for c, a in r[side]:
                    cols.append(c)
                    cfs.append(a)
                offs.append(len(cols))
            return np.array(offs, dtype=np.uint32), np.array(cols if cols else [0], dtype=np.uint32), np.array(cfs if cfs else [0], dtype=np.int64)
        ao, ac, af = flat(0)
        bo, bc, bf = flat(2)
        a0 = np.array([r[1] for r in rows] if rows else [0], dtype=np.int64)
        b0 = np.array([[int(r[3]) & (2**64 - 1), (int(r[3]) >> 64) & (2**64 - 1)] for r in rows] if rows else [[0, 0]], dtype=np.uint64)
        per = np.array([len(st) for st in streams] + [0], dtype=np.uint32)
        self.h = C.c_void_p()
        self.n_streams, self.domain_size, self.n_inputs, self.zero_on_domain = len(streams), domain_size, n_inputs, bool(zero_on_domain)
        _call("jolt_r1cs_rows_create", None, len(streams), domain_size, _p(per), n_inputs, _p(ao), _p(ac), _p(af), _p(a0), _p(bo), _p(bc), _p(bf), _p(b0),
              1 if zero_on_domain else 0, C.byref(self.h))

    @property
    def n_nodes(self):
        return 2 * self.domain_size - 1

    def extension(self):
        """L_i(node): (2D - 1, D) int64"""
        out = np.zeros((self.n_nodes, self.domain_size), dtype=np.int64)
        _call("jolt_r1cs_rows_extension", None, self.h, _p(out))
        return out

    def fold_small(self):
        """the column form of the evaluated nodes: (wa, wb) int64 [node][stream][1 + n_inputs] (JoltError `unsupported` where a folded weight has no int64)"""
        n = C.c_size_t()
        _call("jolt_r1cs_rows_fold_small", None, self.h, None, None, C.byref(n))
        wa = np.zeros((n.value, self.n_streams, 1 + self.n_inputs), dtype=np.int64)
        wb = np.zeros_like(wa)
        _call("jolt_r1cs_rows_fold_small", None, self.h, _p(wa), _p(wb), C.byref(n))
        return wa, wb

    def host_cycle(self, values, kinds, stream, node):
        """jolt_host_r1cs_rows_cycle: one cycle's inputs (Python ints) -> (Az, Bz, Az * Bz) as Python ints"""
        v = np.array([[int(x) & (2**64 - 1), (int(x) >> 64) & (2**64 - 1)] for x in values], dtype=np.uint64)
        k = np.array([Ints.KINDS[q] for q in kinds], dtype=np.int32)
        az, bz, pr, ng = np.zeros(2, dtype=np.uint64), np.zeros(4, dtype=np.uint64), np.zeros(4, dtype=np.uint64), C.c_int32()
        _call("jolt_host_r1cs_rows_cycle", None, self.h, _p(v), _p(k), stream, node, _p(az), _p(bz), _p(pr), C.byref(ng))
        def signed(words, bits):
            x = sum(int(w) << (64 * i) for i, w in enumerate(words))
            return x - (1 << bits) if x >> (bits - 1) else x
        mag = sum(int(w) << (64 * i) for i, w in enumerate(pr))
        return signed(az, 128), signed(bz, 256), -mag if ng.value else mag

    def remainder_weights(self, r0, tau_high):
        """jolt_host_r1cs_rows_remainder_weights -> (fa, fb) [stream][1 + n_inputs], scale"""
        fa, fb, k = fr_array(self.n_streams * (1 + self.n_inputs)), fr_array(self.n_streams * (1 + self.n_inputs)), fr_array(1)
        _call("jolt_host_r1cs_rows_remainder_weights", None, self.h, _p(fr(r0)), _p(fr(tau_high)), _p(fa), _p(fb), _p(k))
        shape = (self.n_streams, 1 + self.n_inputs, 4)
        return fa.reshape(shape), fb.reshape(shape), k[0]

    def destroy(self):
        if self.h:
            lib().jolt_r1cs_rows_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


def host_centered_lagrange_evals(domain_size, r):
    out = fr_array(domain_size)
    _call("jolt_host_centered_lagrange_evals", None, domain_size, _p(fr(r)), _p(out))
    return out


def host_centered_lagrange_kernel(domain_size, x, y):
    out = fr_array(1)
    _call("jolt_host_centered_lagrange_kernel", None, domain_size, _p(fr(x)), _p(fr(y)), _p(out))
    return out[0]


def host_interpolate_to_coeffs(domain_start, values):
    v = fr(values).reshape(-1, 4)
    out = fr_array(v.shape[0])
    _call("jolt_host_interpolate_to_coeffs", None, domain_start, _p(v), v.shape[0], _p(out))
    return out


def host_uniskip_first_round_poly(domain_size, tau_high, t1):
    v = fr(t1).reshape(-1, 4)
    assert v.shape[0] == 2 * domain_size - 1
    out = fr_array(3 * domain_size - 2)
    _call("jolt_host_uniskip_first_round_poly", None, domain_size, _p(fr(tau_high)), _p(v), _p(out))
    return out


def host_prove_uniskip(transcript, coeffs, domain_size, input_claim):
    """jolt_host_prove_uniskip -> (r0, output claim)"""
    c = fr(coeffs).reshape(-1, 4)
    r0, claim = fr_array(1), fr_array(1)
    _call("jolt_host_prove_uniskip", None, transcript.h, _p(c), c.shape[0], domain_size, _p(fr(input_claim)), _p(r0), _p(claim))
    return r0[0], claim[0]


def prove_batch_ops_on(ops, input_claims, coefficients, offsets, max_num_vars, max_degree, transcript, challenge_mode=0, ctx=None):
    """jolt_host_prove_batch_ops_on: prove_batch over operators on a transcript the caller holds"""
    n = len(ops)
    hs = (C.c_void_p * n)(*[o.h for o in ops])
    ic = np.ascontiguousarray(np.stack(input_claims), dtype=np.uint64).reshape(-1, 4)
    co = np.ascontiguousarray(np.stack(coefficients), dtype=np.uint64).reshape(-1, 4)
    offs = (C.c_size_t * n)(*offsets)
    polys, chal = fr_array(max(max_num_vars * (max_degree + 1), 1)), fr_array(max(max_num_vars, 1))
    mclaims, final = fr_array(n), fr_array(1)
    _call("jolt_host_prove_batch_ops_on", ctx, ctx.h if ctx is not None else None, hs, n, _p(ic), _p(co), offs, max_num_vars, max_degree, transcript.h, challenge_mode,
          _p(polys), _p(chal), _p(mclaims), _p(final))
    return dict(polys=polys[: max_num_vars * (max_degree + 1)].reshape(max_num_vars, max_degree + 1, 4), challenges=chal[:max_num_vars], member_claims=mclaims, final_claim=final[0])


def _r1cs_uniskip_sums_rows(self, rows, cols, eq):
    """jolt_r1cs_uniskip_sums_rows: t1 at the 2D - 1 extended nodes (nodes the system marks as vanishing: 0)"""
    out = fr_array(rows.n_nodes)
    _call("jolt_r1cs_uniskip_sums_rows", self, self.h, rows.h, _handles(cols), len(cols), eq.h, _p(out))
    return out


def _stage_spartan_remainder_rows(self, rows, cols, tau, tau_high, r0):
    t = fr(tau).reshape(-1, 4)
    h = C.c_void_p()
    _call("jolt_stage_spartan_remainder_rows_create", self, self.h, rows.h, _handles(cols), len(cols), _p(t), t.shape[0], _p(fr(tau_high)), _p(fr(r0)), C.byref(h))
    return StageOp(self, h, keep=list(cols) + [rows])


def _prove_spartan_stage(self, rows, cols, tau, input_claim, coefficient, transcript):
    """jolt_host_prove_spartan_stage on the caller's transcript -> dict(uniskip_coeffs, r0, uniskip_claim, polys, challenges, final_claim, values)"""
    t = fr(tau).reshape(-1, 4)
    n = t.shape[0] - 1
    D = rows.domain_size
    uc, r0, claim = fr_array(3 * D - 2), fr_array(1), fr_array(1)
    polys, chal, final, values = fr_array(max(n * 4, 1)), fr_array(max(n, 1)), fr_array(1), fr_array(len(cols))
    _call("jolt_host_prove_spartan_stage", self, self.h, rows.h, _handles(cols), len(cols), _p(t), t.shape[0], _p(fr(input_claim)), _p(fr(coefficient)), transcript.h, _p(uc),
          _p(r0), _p(claim), _p(polys), _p(chal), _p(final), _p(values))
    return dict(uniskip_coeffs=uc, r0=r0[0], uniskip_claim=claim[0], polys=polys[: n * 4].reshape(n, 4, 4), challenges=chal[:n], final_claim=final[0], values=values)


Context.r1cs_uniskip_sums_rows = _r1cs_uniskip_sums_rows
Context.stage_spartan_remainder_rows = _stage_spartan_remainder_rows
Context.prove_spartan_stage = _prove_spartan_stage


# ---- precommitted claim reductions (precommitted.hip): the operator pair, its host twin, the table builders ----------------------------------------------------


def _size_array(values):
    v = [int(x) for x in values]
    return (C.c_size_t * max(len(v), 1))(*v), len(v)


def _stage_precommitted_cycle(self, value, eq, aux, cycle_active, cycle_total, address_active=(), address_total=0):
    """jolt_stage_precommitted_cycle_create: the stage-6b cycle phase over COPIES of the resident tables (already in opening-round order)"""
    ca, n_ca = _size_array(cycle_active)
    aa, n_aa = _size_array(address_active)
    h = C.c_void_p()
    _call("jolt_stage_precommitted_cycle_create", self, self.h, value.h, eq.h, _handles(aux), len(aux), ca, n_ca, cycle_total, aa, n_aa, address_total, C.byref(h))
    return StageOp(self, h)


def _stage_precommitted_address(self, cycle_op):
    """jolt_stage_precommitted_address_create: the stage-7 address phase from the carry of a FINISHED cycle operator"""
    h = C.c_void_p()
    _call("jolt_stage_precommitted_address_create", self, self.h, cycle_op.h, C.byref(h))
    return StageOp(self, h)


def stage_host_precommitted(value, eq, aux, cycle_active, cycle_total, address_active=(), address_total=0, length=None):
    """jolt_stage_host_precommitted_create: the same operator over HOST tables (no device, no context).  `length` overrides the table length handed over (refusal tests)"""
    tabs = [np.ascontiguousarray(t, dtype=np.uint64).reshape(-1, 4) for t in [value, eq] + list(aux)]
    ptrs = (C.c_void_p * max(len(tabs) - 2, 1))(*[t.ctypes.data for t in tabs[2:]])
    ca, n_ca = _size_array(cycle_active)
    aa, n_aa = _size_array(address_active)
    h = C.c_void_p()
    _call("jolt_stage_host_precommitted_create", None, _p(tabs[0]), _p(tabs[1]), ptrs, len(tabs) - 2, tabs[0].shape[0] if length is None else length, ca, n_ca, cycle_total,
          aa, n_aa, address_total, C.byref(h))
    return StageOp(None, h)


def stage_host_precommitted_address(cycle_op):
    h = C.c_void_p()
    _call("jolt_stage_host_precommitted_address_create", None, cycle_op.h, C.byref(h))
    return StageOp(None, h)


def host_precommitted_lsb_permutation(perm_be):
    """lsb_permutation -> (old_lsb_to_new_lsb as a list, is_identity)"""
    p, n = _size_array(perm_be)
    out, same = (C.c_size_t * max(n, 1))(), C.c_int32()
    _call("jolt_host_precommitted_lsb_permutation", None, p, n, out, C.byref(same))
    return [int(out[i]) for i in range(n)], bool(same.value)


def host_precommitted_permute_challenges(challenges_be, mapping):
    c = fr(challenges_be).reshape(-1, 4)
    m, n = _size_array(mapping)
    out = fr_array(max(n, 1))
    _call("jolt_host_precommitted_permute_challenges", None, _p(c), c.shape[0], m, _p(out))
    return out[:n]


def _table_permute_bits(self, table, old_lsb_to_new_lsb):
    m, n = _size_array(old_lsb_to_new_lsb)
    h = C.c_void_p()
    _call("jolt_table_permute_bits", self, self.h, table.h, m, n, C.byref(h))
    return Table(self, h)


def _eq_evals_shifted(self, r, start_index, length):
    r = fr(r).reshape(-1, 4)
    h = C.c_void_p()
    _call("jolt_eq_evals_shifted", self, self.h, _p(r), r.shape[0], start_index, length, C.byref(h))
    return Table(self, h)


def _table_outer(self, lane_weights, cycle_table, order):
    w = fr(lane_weights).reshape(-1, 4)
    h = C.c_void_p()
    _call("jolt_table_outer", self, self.h, _p(w), w.shape[0], cycle_table.h, order, C.byref(h))
    return Table(self, h)


Context.stage_precommitted_cycle = _stage_precommitted_cycle
Context.stage_precommitted_address = _stage_precommitted_address
Context.table_permute_bits = _table_permute_bits
Context.eq_evals_shifted = _eq_evals_shifted
Context.table_outer = _table_outer


# ---- TESTS ONLY: the device twins of the host forms (device_probe.hip) ---------------------------------------------------------------------------------------
# One call = one launch over n operand tuples.  Arrays may be None and `n` / `out` may be given, so that the suite can make the calls the entries refuse; a refused
# call raises JoltError and leaves `out` as it was.
def _rows(a, width, dtype=np.uint64):
    return np.ascontiguousarray(a, dtype=dtype).reshape(-1, width) if a is not None else None


def _probe_n(n, *arrays):
    return n if n is not None else next(a.shape[0] for a in arrays if a is not None)


def host_field_op(field, op, a, b=None):
    """PROBE_* over (n, 4) operand arrays on the host, with the device's multiplication algorithm wherever the device multiplies; field 0 = Fr, 1 = Fq"""
    a, b = _rows(a, 4), _rows(b, 4)
    out = fr_array(a.shape[0])
    _call("jolt_host_field_op", None, field, op, _p(a), _p(b), a.shape[0], _p(out))
    return out


def probe_field_op(ctx, field, op, a, b=None, n=None, out=None):
    a, b = _rows(a, 4), _rows(b, 4)
    n = _probe_n(n, a, b)
    out = fr_array(n) if out is None else out
    _call("jolt_probe_field_op", ctx, ctx.h if ctx else None, field, op, _p(a), _p(b), n, _p(out))
    return out


def probe_fq_limb_op(ctx, op, a, b=None, c=None, d=None, n=None, out=None):
    a, b, c, d = (_rows(x, 4) for x in (a, b, c, d))
    n = _probe_n(n, a, b, c, d)
    out = fr_array(n) if out is None else out
    _call("jolt_probe_fq_limb_op", ctx, ctx.h if ctx else None, op, _p(a), _p(b), _p(c), _p(d), n, _p(out))
    return out


def probe_g1xl_add_paths(ctx, acc, q, negate):
    """host_g1xl_add_paths over n tuples: acc (n, 36), q (n, 18) uint32 limbs, negate (n,); the same dict with a leading axis of n"""
    acc, q = _rows(acc, 36, np.uint32), _rows(q, 18, np.uint32)
    neg = np.ascontiguousarray(negate, dtype=np.int32).reshape(-1)
    n = acc.shape[0]
    common, full, step = (np.zeros((n, 4, 9), dtype=np.uint32) for _ in range(3))
    canon, sus = np.zeros((n, 2, 4, 8), dtype=np.uint32), np.zeros(n, dtype=np.int32)
    _call("jolt_probe_g1xl_add_paths", ctx, ctx.h, _p(acc), _p(q), _p(neg), n, _p(common), _p(full), _p(step), _p(sus), _p(canon))
    return {"common": common, "full": full, "step": step, "suspect": sus != 0, "canon_common": canon[:, 0], "canon_full": canon[:, 1]}


def probe_fq2_op(ctx, op, a, b=None, n=None, out=None):
    a, b = _rows(a, 8), _rows(b, 8)
    n = _probe_n(n, a, b)
    out = np.zeros((n, 8), dtype=np.uint64) if out is None else out
    _call("jolt_probe_fq2_op", ctx, ctx.h if ctx else None, op, _p(a), _p(b), n, _p(out))
    return out


def probe_g2_op(ctx, op, p, q=None):
    """PROBE_G2_ADD / _DOUBLE -> (n, 24) points, PROBE_G2_EQ -> (n,) bool"""
    p, q = _rows(p, 24), _rows(q, 24)
    n = p.shape[0]
    out, equal = np.zeros((n, 24), dtype=np.uint64), np.zeros(n, dtype=np.int32)
    _call("jolt_probe_g2_op", ctx, ctx.h, op, _p(p), _p(q), n, _p(out), _p(equal))
    return equal != 0 if op == PROBE_G2_EQ else out  # noqa: F821 (the header's constant)


def probe_fq12_op(ctx, op, a, b=None, n=None, out=None):
    a, b = _rows(a, 48), _rows(b, 48)
    n = _probe_n(n, a, b)
    out = np.zeros((n, 48), dtype=np.uint64) if out is None else out
    _call("jolt_probe_fq12_op", ctx, ctx.h if ctx else None, op, _p(a), _p(b), n, _p(out))
    return out


def probe_suffix_mle(ctx, kinds, bits, lengths, n=None, out=None):
    """host_suffix_mle over n tuples; bits are Python ints of up to 128 bits"""
    kind = np.ascontiguousarray(kinds, dtype=np.uint32)
    lo = np.array([int(b) & (2**64 - 1) for b in bits], dtype=np.uint64)
    hi = np.array([(int(b) >> 64) & (2**64 - 1) for b in bits], dtype=np.uint64)
    length = np.ascontiguousarray(lengths, dtype=np.uint32)
    n = kind.shape[0] if n is None else n
    out = np.zeros(n, dtype=np.uint64) if out is None else out
    _call("jolt_probe_suffix_mle", ctx, ctx.h if ctx else None, _p(kind), _p(lo), _p(hi), _p(length), n, _p(out))
    return out


def probe_dory_fr_digits(ctx, scalars, c, W, n=None, out=None):
    """host_dory_fr_digits over n scalars: ((n, W) signed digits as int64, (n,) bool negative)"""
    s = _rows(scalars, 4)
    n = _probe_n(n, s)
    digits = np.zeros((n, max(W, 1)), dtype=np.uint32) if out is None else out
    neg = np.zeros(digits.shape[0], dtype=np.uint32)
    _call("jolt_probe_dory_fr_digits", ctx, ctx.h, _p(s), n, c, W, _p(digits), _p(neg))
    mag = (digits & np.uint32(0x7FFFFFFF)).astype(np.int64)
    return np.where(digits >> np.uint32(31) != 0, -mag, mag), neg != 0


def _small_column(ints, kind):
    """Python ints -> the column's words: one uint64 per term, (lo, hi) two's complement for INT_I128"""
    if kind == INT_I128:  # noqa: F821
        return np.array([[int(x) & (2**64 - 1), (int(x) >> 64) & (2**64 - 1)] for x in ints], dtype=np.uint64).reshape(-1, 2)
    return np.array([int(x) & (2**64 - 1) for x in ints], dtype=np.uint64)


def host_small_scalar_dots(values, ints, kind, offsets):
    """out[i] = sum of values[k] * ints[k] over offsets[i] <= k < offsets[i + 1] through the device's small-scalar accumulator, on the host; kind = INT_U64 / _I64 / _I128"""
    v, z, off = _rows(values, 4), _small_column(ints, kind), np.ascontiguousarray(offsets, dtype=np.uint64)
    out = fr_array(off.shape[0] - 1)
    _call("jolt_host_small_scalar_dots", None, _p(v), _p(z), kind, _p(off), v.shape[0], off.shape[0] - 1, _p(out))
    return out


def probe_small_scalar_dots(ctx, values, ints, kind, offsets, n_terms=None, out=None):
    v, z, off = _rows(values, 4), _small_column(ints, kind), np.ascontiguousarray(offsets, dtype=np.uint64)
    out = fr_array(off.shape[0] - 1) if out is None else out
    _call("jolt_probe_small_scalar_dots", ctx, ctx.h if ctx else None, _p(v), _p(z), kind, _p(off), v.shape[0] if n_terms is None else n_terms, off.shape[0] - 1, _p(out))
    return out
