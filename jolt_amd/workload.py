"""Synthetic "sha3-shaped" prover workload for the sumcheck hot path.

The reference sizes a sha3 trace as 4330 cycles per hash at 90 % fill of 2^scale
(crates/jolt-prover/src/profile.rs:80-84,547-551) and then runs, per stage, one batched sumcheck over the cycle
domain.  Without the Rust toolchain no real trace exists here, so the workload is the member catalogue of
SURVEY.md section 8 a13 -- every T-sized, cycle-domain relation of stages 2..6b with the reference's summand shape,
degree and table count -- over synthetic tables of the right kind (u64-valued witness columns promoted on the
device, eq / eq+1 / LT tables expanded on the device from random points).  Each relation is written in the fused
"product of linear combinations" form the optimized tier uses, as a descriptor for the generic device member.

This module only DESCRIBES the workload (numpy + descriptors); bench.py and the tests instantiate it on the GPU
through the C ABI, and (tests / cpu_baseline only) on the CPU oracle.
"""
import os

import numpy as np

P_TOP = 0x30644E72E131A029


def rand_fr(n, rng):
    a = rng.integers(0, 2**64, size=(n, 4), dtype=np.uint64)
    a[:, 3] = a[:, 3] % np.uint64(P_TOP)
    return a


class TableSpec:
    """kind: 'u64' (witness column, values < 2^bits), 'eq', 'eq1' (eq+1), 'lt' -- derived tables carry their point;
    'onehot': an address-folded one-hot selector column ra(j) = eq(point, .)[data[j]] -- `data` = uint8 hot indices in
    [0, 2^len(point)) or 0xFF on a cold cycle, `point` = the chunk point (log_k_chunk coordinates)."""

    def __init__(self, name, kind, bits=64, point=None, data=None):
        self.name, self.kind, self.bits, self.point, self.data = name, kind, bits, point, data


class MemberSpec:
    def __init__(self, name, stage, degree, tables, groups=None, split_eq=None, uniform=None, eq_inner=None, fused=None, reference=""):
        self.name, self.stage, self.degree, self.tables = name, stage, degree, tables
        self.groups = groups        # LC form: [[(const|None, [(coeff, local_table_idx), ...]), ...], ...]
        self.split_eq = split_eq    # (a_idx, b_idx, w) for the split-eq product member
        self.uniform = uniform      # (V, F, [coeff symbols]): tables[0] is eq(w,.), tables[1 + v*F + i] the product tables;
                                    # the device serves eq from split tables (split-eq uniform member), the oracle uses `groups`
        self.eq_inner = eq_inner    # (dq, inner groups over tables[1:]): the summand is eq(tables[0]) * q with the eq weight factored out
                                    # on the device (jolt_member_create_split_eq_lc); `groups` stays the oracle's full form
        self.fused = fused          # linear-leaf fusion (optimized/inc_claim_reduction.rs:6-13,68-89): ([(fused name, [(coeff, local idx), ..]) ..],
                                    # device table list (names or fused names), device groups) -- A = sum_i s_i * eq(p_i) built once per proof
        self.reference = reference  # reference file of the relation


def build(n_vars, seed=2026, d_ram=4, n_instruction_ra=32):
    """Returns (tables: dict name -> TableSpec, members: [MemberSpec]) for a trace of T = 2^n_vars cycles."""
    rng = np.random.default_rng(seed)
    T = 1 << n_vars
    tables = {}
    one = None  # resolved by the instantiator (Montgomery one)

    def wit(name, bits=64):
        hi = 2**bits if bits < 64 else 2**64
        tables[name] = TableSpec(name, "u64", bits, data=rng.integers(0, hi, size=T, dtype=np.uint64))
        return name

    def derived(name, kind):
        tables[name] = TableSpec(name, kind, point=rand_fr(n_vars, rng))
        return name

    def onehot(name, cold=0.0, log_k=4, cold_mask=None):
        """committed RA polynomial chunk, address-folded: K = 2^log_k = 16 (crates/jolt-prover/src/config.rs:175-186).  cold_mask: the chunks of ONE address
        (the RAM address of a cycle) are cold together -- a cycle either accesses memory or does not"""
        idx = rng.integers(0, 1 << log_k, size=T, dtype=np.uint8)
        if cold_mask is not None:
            idx[cold_mask] = 0xFF
        elif cold:
            idx[rng.random(T) < cold] = 0xFF
        tables[name] = TableSpec(name, "onehot", point=rand_fr(log_k, rng), data=idx)
        return name

    def scalar():
        return rand_fr(1, rng)[0]

    def powers(g, k):
        return ("powers", g, k)  # resolved lazily: [1, g, g^2, ...] needs field multiplication

    members = []

    # ---- stage 2: instruction_claim_reduction  eq(tau,j) * (o1 + g o2 + ... + g^4 o5)          deg 2, 6 tables
    t = [derived("s2.eq", "eq")] + [wit(f"s2.o{k}") for k in range(5)]
    members.append(MemberSpec("instruction_claim_reduction", 2, 2, t,
                              groups=[[(None, [("one", 0)]), (None, [(("gpow", 0, k), 1 + k) for k in range(5)])]],
                              eq_inner=(1, [[(None, [(("gpow", 0, k), k) for k in range(5)])]]),
                              reference="crates/jolt-kernels/src/optimized/instruction_claim_reduction.rs"))
    # ---- stage 3: spartan_shift  eq+1(tau,j)*(upc + g pc + g^2 virt + g^3 first) + g^4 eq+1(r,j)*(1 - noop)   deg 2, 7 tables
    t = [derived("s3.eq1a", "eq1"), wit("s3.upc"), wit("s3.pc"), wit("s3.virt", 1), wit("s3.first", 1), derived("s3.eq1b", "eq1"),
         wit("s3.noop", 1)]
    members.append(MemberSpec("spartan_shift", 3, 2, t,
                              groups=[[(None, [("one", 0)]), (None, [(("gpow", 1, k), 1 + k) for k in range(4)])],
                                      [(None, [(("gpow", 1, 4), 5)]), ("one", [("minus_one", 6)])]],
                              reference="crates/jolt-kernels/src/reference/spartan_shift.rs"))
    # ---- stage 3: instruction_input  eq*((f1 rs2 + f2 imm) + g (f3 rs1 + f4 upc))                deg 3, 9 tables
    t = [derived("s3.eq_in", "eq"), wit("s3.f1", 1), wit("s3.rs2"), wit("s3.f2", 1), wit("s3.imm"), wit("s3.f3", 1), wit("s3.rs1"),
         wit("s3.f4", 1), wit("s3.upc2")]
    members.append(MemberSpec("instruction_input", 3, 3, t,
                              groups=[[(None, [("one", 0)]), (None, [("one", 1)]), (None, [("one", 2)])],
                                      [(None, [("one", 0)]), (None, [("one", 3)]), (None, [("one", 4)])],
                                      [(None, [(("gpow", 2, 1), 0)]), (None, [("one", 5)]), (None, [("one", 6)])],
                                      [(None, [(("gpow", 2, 1), 0)]), (None, [("one", 7)]), (None, [("one", 8)])]],
                              eq_inner=(2, [[(None, [("one", 0)]), (None, [("one", 1)])],
                                            [(None, [("one", 2)]), (None, [("one", 3)])],
                                            [(None, [(("gpow", 2, 1), 4)]), (None, [("one", 5)])],
                                            [(None, [(("gpow", 2, 1), 6)]), (None, [("one", 7)])]]),
                              reference="crates/jolt-kernels/src/optimized/instruction_input.rs:1-22"))
    # ---- stage 3: registers_claim_reduction  eq*(rd_w + g rs1 + g^2 rs2)                        deg 2, 4 tables
    t = [derived("s3.eq_reg", "eq"), wit("s3.rd_w"), wit("s3.rs1v"), wit("s3.rs2v")]
    members.append(MemberSpec("registers_claim_reduction", 3, 2, t,
                              groups=[[(None, [("one", 0)]), (None, [(("gpow", 3, k), 1 + k) for k in range(3)])]],
                              eq_inner=(1, [[(None, [(("gpow", 3, k), k) for k in range(3)])]]),
                              reference="crates/jolt-kernels/src/reference/registers_claim_reduction.rs"))
    # ---- stage 4: ram_val_check  inc(j) * ra(j) * (LT(j,r) + g)                                  deg 3, 3 tables
    t = [wit("s4.inc"), derived("s4.ra", "eq"), derived("s4.lt", "lt")]
    members.append(MemberSpec("ram_val_check", 4, 3, t,
                              groups=[[(None, [("one", 0)]), (None, [("one", 1)]), (("gpow", 4, 1), [("one", 2)])]],
                              reference="crates/jolt-kernels/src/reference/ram_val_check.rs"))
    # ---- stage 5: registers_val_evaluation  LT(j,r) * rd_inc(j) * rd_wa(r_addr,j)                deg 3, 3 tables
    t = [derived("s5.lt", "lt"), wit("s5.rd_inc"), derived("s5.rd_wa", "eq")]
    members.append(MemberSpec("registers_val_evaluation", 5, 3, t,
                              groups=[[(None, [("one", 0)]), (None, [("one", 1)]), (None, [("one", 2)])]],
                              reference="crates/jolt-kernels/src/reference/registers_val_evaluation.rs"))
    # ---- stage 5: ram_ra_claim_reduction  (eq1 + g eq2 + g^2 eq3)(j) * ra(r_addr,j)              deg 2, 4 tables
    t = [derived("s5.eq1", "eq"), derived("s5.eq2", "eq"), derived("s5.eq3", "eq"), derived("s5.ra", "eq")]
    members.append(MemberSpec("ram_ra_claim_reduction", 5, 2, t,
                              groups=[[(None, [(("gpow", 5, k), k) for k in range(3)]), (None, [("one", 3)])]],
                              fused=([("s5.eqA", [(("gpow", 5, k), k) for k in range(3)])], ["s5.eqA", "s5.ra"],
                                     [[(None, [("one", 0)]), (None, [("one", 1)])]]),
                              reference="crates/jolt-kernels/src/reference/ram_ra_claim_reduction.rs"))
    # ---- stage 6b: inc_claim_reduction  (eq1 + g eq2) RamInc + g^2 (eq3 + g eq4) RdInc           deg 2, 6 tables
    t = [derived("s6.eq1", "eq"), derived("s6.eq2", "eq"), wit("s6.ram_inc"), derived("s6.eq3", "eq"), derived("s6.eq4", "eq"),
         wit("s6.rd_inc")]
    members.append(MemberSpec("inc_claim_reduction", 6, 2, t,
                              groups=[[(None, [("one", 0), (("gpow", 6, 1), 1)]), (None, [("one", 2)])],
                                      [(None, [(("gpow", 6, 2), 3), (("gpow", 6, 3), 4)]), (None, [("one", 5)])]],
                              fused=([("s6.eqA", [("one", 0), (("gpow", 6, 1), 1)]), ("s6.eqB", [(("gpow", 6, 2), 3), (("gpow", 6, 3), 4)])],
                                     ["s6.eqA", "s6.ram_inc", "s6.eqB", "s6.rd_inc"],
                                     [[(None, [("one", 0)]), (None, [("one", 1)])], [(None, [("one", 2)]), (None, [("one", 3)])]]),
                              reference="crates/jolt-kernels/src/optimized/inc_claim_reduction.rs:6-13,68-89"))
    # ---- stage 6b: ram_hamming_booleanity  eq(r,j) * (H^2 - H) = eq * H * (H - 1)                deg 3, split-eq member
    t = [wit("s6.H", 1), "s6.H_minus_1"]
    tables["s6.H_minus_1"] = TableSpec("s6.H_minus_1", "i64", data=tables["s6.H"].data.astype(np.int64) - 1)
    members.append(MemberSpec("ram_hamming_booleanity", 6, 3, t, split_eq=(0, 1, rand_fr(n_vars, rng)),
                              reference="crates/jolt-kernels/src/optimized/ram_hamming_booleanity.rs:111-135"))
    # ---- stage 6b: ram_ra_virtualization  eq(r,j) * prod_{i<d} ra_i                             deg 1+d, 1+d tables
    #      ra_i(j) = eq(r_chunk_i, chunk_i(j)): one-hot selector columns, ~40 % cold cycles (specs/byte-addressable-memory.md:119)
    ram_cold = rng.random(T) < 0.4
    t = [derived("s6.eq_rv", "eq")] + [onehot(f"s6.ram_ra{i}", cold_mask=ram_cold) for i in range(d_ram)]
    members.append(MemberSpec("ram_ra_virtualization", 6, 1 + d_ram, t,
                              groups=[[(None, [("one", i)]) for i in range(1 + d_ram)]],
                              uniform=(1, d_ram, ["one"]) if 2 <= d_ram <= 4 else None,
                              reference="crates/jolt-kernels/src/reference/ram_ra_virtualization.rs"))
    # ---- stage 6b: instruction_ra_virtualization  eq * sum_v g^v prod_{i<4} ra_{4v+i}            deg 5, 1+32 tables
    t = [derived("s6.eq_iv", "eq")] + [onehot(f"s6.ins_ra{i}") for i in range(n_instruction_ra)]
    members.append(MemberSpec("instruction_ra_virtualization", 6, 5, t,
                              groups=[[(None, [(("gpow", 7, v), 0)])] + [(None, [("one", 1 + 4 * v + i)]) for i in range(4)]
                                      for v in range(n_instruction_ra // 4)],
                              uniform=(n_instruction_ra // 4, 4, [("gpow", 7, v) for v in range(n_instruction_ra // 4)]),
                              reference="crates/jolt-kernels/src/reference/instruction_ra_virtualization.rs"))
    gammas = [scalar() for _ in range(8)]
    return tables, members, gammas


class Resolver:
    """Turns symbolic coefficients ('one', 'minus_one', ('gpow', g, k)) into Montgomery limbs with a caller-supplied
    field multiplication (device host-helper for the product, oracle for the CPU baseline)."""

    def __init__(self, gammas, one, mul, neg):
        self.one, self.mul, self.negf = one, mul, neg
        self.gammas = gammas
        self.cache = {}

    def coeff(self, c):
        if isinstance(c, np.ndarray):
            return c
        if c is None:
            return None
        if c == "one":
            return self.one
        if c == "minus_one":
            return self.negf(self.one)
        if isinstance(c, tuple) and c[0] == "gpow":
            key = (c[1], c[2])
            if key not in self.cache:
                v = self.one
                for _ in range(c[2]):
                    v = self.mul(v, self.gammas[c[1]])
                self.cache[key] = v
            return self.cache[key]
        raise ValueError(c)

    def groups(self, groups):
        return [[(self.coeff(const), [(self.coeff(c), ti) for c, ti in entries]) for const, entries in g] for g in groups]


def expand_to_flat_terms(groups, mul, one):
    """Distribute a resolved LC-form summand into the reference tier's flat Expr terms [(coeff, [table idx...])]
    (constants multiply into the coefficient).  Used by the tests to compare the fused device member with the
    oracle's naive member."""
    terms = []
    for g in groups:
        partial = [(one, [])]
        for const, entries in g:
            nxt = []
            for c0, f0 in partial:
                if const is not None:
                    nxt.append((mul(c0, const), list(f0)))
                for c, ti in entries:
                    nxt.append((mul(c0, c), f0 + [ti]))
            partial = nxt
        terms.extend(partial)
    return terms


# ---------------------------------------------------------------------------------------------------------------------
# GPU instantiation through the C ABI (product path; no oracle involved)
# ---------------------------------------------------------------------------------------------------------------------
class DeviceWorkload:
    """One synthetic proof after another on the device, with the life cycle of the reference prover
    (crates/jolt-prover/src/dory/prover.rs:133-252; metric window crates/jolt-prover/src/profile.rs:590-601):

      resident inputs (constructor, untimed -- "inputs already in HBM"): the witness columns as 64-bit integers, the hot indices
        of the one-hot RA columns, the SRS;
      prepare()  -- PrepareKernel::prepare of every member (crates/jolt-kernels/src/backend.rs:98-111): witness promotion to field
        tables, every T-sized derived table (eq / eq+1 / LT expansions from the stage's points, the address tables of the one-hot
        columns, linear-leaf fusions through jolt_rlc), descriptor upload, split-eq tables;
      commit()   -- stage 0: the committed columns over the shared K x T commitment grid (pcs="grid");
      prove()    -- stages 2..6b: one batched sumcheck per stage through jolt_host_prove_batch;
      open()     -- stage 8: joint polynomial of the homomorphic batch + ONE HyperKZG opening (crates/jolt-openings/src/schemes.rs:487-524);
      release()  -- drop members and per-proof tables (back into the context's pool).
    step() runs all of them: that is one timed step of bench.py.  The stage points are fixed per workload (the same tables are
    REBUILT every step); the input claims -- in a real proof the previous stage's output claims -- are computed once.

    pcs: None (sumcheck only: BASELINE configs[1]) or "grid" (configs[2]: every committed polynomial lives on the 2^(log_k + n_vars)
    commitment grid of crates/jolt-kernels/src/commitment.rs:86-130 -- the two dense increment columns at address 0, the one-hot
    RA columns as 0/1 coefficients -- committed with HyperKZG and opened jointly at one point) or "dory" (the same columns over the same
    grid under the reference's production scheme: commit() is a dory_commit.DoryWitnessCommitment -- resident tier-1 hints, tier 2 as one
    product batch -- and open() is HomomorphicBatch::prove_batch as one library call, jolt_host_dory_prove_batch, over the statement's claims
    `opening_claims`, which one launch over the witness columns computes at construction; dory_bases= plants the setup's bases, otherwise
    jolt_amd/dory_setup.py generates 2^sigma per group from the seed; dory_blocks= adds the polynomials of stage 8 that are field elements -- advice, bytecode
    chunks, the program image -- as block-embedded columns after the trace's: host arrays (2^m, 4) or log2 sizes m to draw from the seed, committed by
    jolt_dory_hints_rows_fr, their claims from jolt_dory_evaluate_blocks, opened with the trace by jolt_host_dory_prove_batch_blocks; dory_order="address_major"
    (with dory_log_extra) commits and opens the trace in the other placement, open_point then in that grid's order)."""

    def __init__(self, ctx, n_vars, seed=2026, pcs=None, srs=None, fixed_base=True, extended=False, witness_upload=False, ram_addresses="uniform", **kw):
        from . import ffi
        if pcs == "dory" and n_vars < 4:  # sigma = ceil((4 + n_vars) / 2) > n_vars: a matrix row wider than one address's cycles (refused before anything is uploaded)
            raise ValueError("pcs='dory' needs n_vars >= 4")
        # pcs="dory": the polynomials of stage 8 that are field elements and not trace columns (advice, bytecode chunks, the program image), embedded top-left in the
        # grid: host arrays (2^m, 4) of canonical field elements, or m itself (generated from the seed); the trace placement; the widening of an address-major grid
        dory_blocks, dory_order, dory_log_extra = list(kw.pop("dory_blocks", ())), kw.pop("dory_order", "cycle_major"), int(kw.pop("dory_log_extra", 0))
        if pcs == "dory":  # refused before anything is uploaded
            dory_blocks = self._check_dory_shape(n_vars, seed, dory_blocks, dory_order, dory_log_extra)
        elif dory_blocks or dory_order != "cycle_major" or dory_log_extra:
            raise ValueError("dory_blocks, dory_order and dory_log_extra belong to pcs='dory'")
        self.ctx, self.n_vars, self.ffi, self.pcs, self._seed = ctx, n_vars, ffi, pcs, seed
        # witness_upload: every step STARTS from the packed per-cycle rows in host memory (RowSource::rows() + WitnessBundle::from_row windows,
        # crates/jolt-witness/src/consumer.rs:129-143, crates/jolt-kernels/src/optimized/rows.rs:22-72): one H2D copy of the rows, the typed columns and hot
        # indices extracted on the device (jolt_rows_upload, jolt_ints_from_rows, jolt_onehot_from_rows).  Default: the witness is resident ("inputs in HBM").
        self.witness_upload = bool(witness_upload)
        self.witness_pinned = witness_upload in ("pinned", "overlapped")  # the row buffer in page-locked memory (jolt_host_pinned_alloc) instead of pageable numpy memory
        # "overlapped": the NEXT proof's rows are copied (jolt_rows_upload_begin, on the context's copy stream) while the current proof runs -- a prover fed by a tracer
        # that is one trace ahead; every proof still starts from host memory, the copy is simply no longer on its critical path
        self.witness_overlapped = witness_upload == "overlapped"
        self._rows_in_flight = None
        # extended: the stage 1 / 2 / 5 operators that are not plain cycle-domain relations (Spartan outer / product, the sparse RAM read-write
        # matrix, the instruction read-RAF scans + cycle rounds: jolt_amd/stages.py) inside every step, over their own resident inputs
        self.ext, self.ext_ctx, self._stage_worker, self._stage_slots = None, None, None, []
        if extended:
            import os
            from .stages import DeviceExtended
            # The stage operators live on THEIR OWN context (own stream, scratch and pool) and are driven from a worker thread, so that the operators of protocol stage k run
            # beside stage k's batched sumcheck of the catalogue -- the reference proves a stage's members as one batch; nothing crosses a stage boundary (prove_stages).
            # JOLT_STAGE_CONCURRENCY=0: one context, the operators and the catalogue one after the other (the structure of rounds 3 - 5, for an A/B).
            # JOLT_STAGE_CONTEXTS (default 2): independent operator chains of one stage (RAM read-write beside the product remainder and the RAM address-domain relations;
            # bytecode read+RAF beside the booleanity phases) each get a context and a thread.
            if os.environ.get("JOLT_STAGE_CONCURRENCY", "1") != "0":
                from concurrent.futures import ThreadPoolExecutor
                self.ext_ctx = ffi.Context(ctx.device_id)
                n_slots = max(1, min(2, int(os.environ.get("JOLT_STAGE_CONTEXTS", "2"))))
                self._stage_slots = [(ThreadPoolExecutor(max_workers=1), self.ext_ctx if k == 0 else ffi.Context(ctx.device_id)) for k in range(n_slots)]
                self._stage_worker = self._stage_slots[0][0]
            self.ext = DeviceExtended(self.ext_ctx or ctx, n_vars, seed, ram_addresses=ram_addresses)  # "hotset": a btreemap-like skewed RAM / register address stream
            for pool, slot_ctx in self._stage_slots:
                pool.submit(lambda c=slot_ctx: (c.bind_thread(), self.ext.bind_context(c))).result()
        dory_bases = kw.pop("dory_bases", None)  # pcs="dory": dict(gamma1, gamma2, h1, h2) of host arrays (jolt_amd/dory_setup.py); None: generated from the seed
        self.tables_spec, self.members_spec, gammas = build(n_vars, seed, **kw)
        one = ffi.host_fr_from_u64(1)
        zero = np.zeros(4, dtype=np.uint64)
        self.resolver = Resolver(gammas, one, ffi.host_fr_mul, lambda x: ffi.host_fr_sub(zero, x))
        self.one = one
        # which tables are materialised per proof: eq tables that only feed split-eq members never are; one-hot selector columns
        # that only feed uniform members stay index-encoded (1 byte per cycle, LazyFoldedRa)
        skip = {ms.tables[0] for ms in self.members_spec if ms.uniform is not None}
        skip -= {t for ms in self.members_spec for t in (ms.tables if ms.uniform is None else ms.tables[1:])}
        self._lazy = lambda ms: ms.uniform is not None and n_vars >= 4 and all(self.tables_spec[t].kind == "onehot" for t in ms.tables[1:])
        skip |= {t for ms in self.members_spec if self._lazy(ms) for t in ms.tables[1:]}
        skip |= {ms.tables[0] for ms in self.members_spec if ms.eq_inner is not None}  # eq weight factored out: never materialised
        used = lambda ms: ms.tables[1:] if (ms.uniform is not None or ms.eq_inner is not None) else ms.tables
        skip -= {t for ms in self.members_spec if not self._lazy(ms) for t in used(ms)}
        # Compact-scalar witness columns (the optimized tier's Polynomial<u64>: round 0 off the integers, bind_to_field on the first bind,
        # crates/jolt-poly/src/dense.rs:129-142): u64 columns that only feed descriptor-driven members are never promoted -- the members read the resident
        # integers (jolt_member_create_lc_small).  Not: the two committed increment columns (commit and the joint polynomial need them as field tables) and the
        # split-eq product member's columns.
        int_capable = lambda ms: ms.uniform is None and ms.fused is None and ms.split_eq is None
        small = {t for ms in self.members_spec if int_capable(ms) for t in (ms.tables[1:] if ms.eq_inner is not None else ms.tables)
                 if self.tables_spec[t].kind == "u64"}
        small -= {t for ms in self.members_spec if not int_capable(ms) for t in ms.tables}
        small -= {"s6.ram_inc", "s6.rd_inc"}
        self._small = small
        skip |= small
        self._skip = skip
        # ---- resident inputs
        self.ints = {}
        for name, spec in self.tables_spec.items():
            if name in skip and name not in self._small:
                continue
            if spec.kind in ("u64", "i64"):
                self.ints[name] = ctx.ints(spec.data.astype(np.uint64 if spec.kind == "u64" else np.int64))
        self.sources = {}  # member index -> OneHot (lazy members); dense one-hot tables get theirs in _make_table
        for i, ms in enumerate(self.members_spec):
            if self._lazy(ms):
                specs = [self.tables_spec[t] for t in ms.tables[1:]]
                self.sources[i] = ctx.onehot(np.stack([sp.data for sp in specs]), 1 << len(specs[0].point))
        rng = np.random.default_rng(seed + 1)
        self.batch_coeffs = [rand_fr(1, rng)[0] for _ in self.members_spec]
        self.n_tables = sum(len(ms.tables) for ms in self.members_spec)
        self.n_onehot = sum(len(ms.tables) - 1 for ms in self.members_spec if self._lazy(ms))
        self.stages = {}
        for i, ms in enumerate(self.members_spec):
            self.stages.setdefault(ms.stage, []).append(i)
        # ---- PCS side (pcs="grid")
        self.srs, self.own_srs, self.grid_pairs_bytes = srs, False, 0
        if pcs == "grid":
            self.log_k = 4
            assert all(len(self.tables_spec[t].point) == self.log_k for ms in self.members_spec if self._lazy(ms) for t in ms.tables[1:])
            self.grid_vars = self.log_k + n_vars
            self.committed_dense = ["s6.ram_inc", "s6.rd_inc"]  # RamInc, RdInc (CommittedColumnsWitness, crates/jolt-kernels/src/commitment.rs:25-32)
            if self.srs is None:
                prng = np.random.default_rng(seed + 2)
                self.beta = rand_fr(1, prng)[0]
                self.srs = ctx.srs_setup_from_secret(self.beta, 1 << self.grid_vars, G1_GENERATOR)
                self.own_srs = True
                ctx.synchronize()
                if fixed_base and self.grid_vars >= 12:  # setup-time (like the SRS itself): window-precomputed bases for the big MSMs
                    ctx.srs_precompute_windows(self.srs)
                    # ... and the grid's pair tables beside them (a function of the SRS, K and T alone): shift 0 serves the commitment's sums of bases, shifts
                    # 1 .. linear_levels() the opening hint's; JOLT_GRID_PAIR_SHIFTS ("" or e.g. "0,1") overrides the set for A/B runs
                    import os
                    shifts = os.environ.get("JOLT_GRID_PAIR_SHIFTS")
                    shifts = range(self.linear_levels() + 1) if shifts is None else [int(s) for s in shifts.split(",") if s.strip()]
                    if len(shifts):
                        self.grid_pairs_bytes = sum(ctx.srs_precompute_grid_pairs(self.srs, 1 << self.log_k, 1 << n_vars, shifts).values())
            prng = np.random.default_rng(seed + 3)
            n_oh = sum(self.sources[i].n_polys for i in sorted(self.sources))
            self.rlc_onehot = rand_fr(n_oh, prng)
            self.rlc_dense = rand_fr(len(self.committed_dense), prng)
            self.open_point = rand_fr(self.grid_vars, prng)
        elif pcs == "dory":
            # The same committed columns over the same cycle-major grid, under the reference's production scheme: the grid is a 2^nu x 2^sigma matrix
            # (crates/jolt-dory/src/scheme.rs:242-243) and the setup is 2^sigma bases per group -- built here, once, untimed, like the SRS of pcs="grid".
            from . import dory_setup
            from .dory_proof import DoryProofSetup
            self.log_k = 4
            assert all(len(self.tables_spec[t].point) == self.log_k for ms in self.members_spec if self._lazy(ms) for t in ms.tables[1:])
            self.dory_order, self.dory_log_extra = dory_order, dory_log_extra
            self.grid_vars = self.log_k + n_vars + dory_log_extra
            self.committed_dense = ["s6.ram_inc", "s6.rd_inc"]
            self.dory_sigma = (self.grid_vars + 1) // 2
            self.dory_nu = self.grid_vars - self.dory_sigma
            width = 1 << self.dory_sigma
            bases = dory_setup.check(dory_bases) if dory_bases is not None else dory_setup.generate(ctx, width, seed + 2)
            if bases["gamma1"].shape[0] < width:
                raise ValueError("dory_bases holds fewer than 2^sigma bases per group")
            # ONE setup object over the bases (jolt_dory_setup): the commitment's tier 2 goes through its prepared Gamma2 (DoryLibSetup.tier2) and the opening through
            # the same handle, so the bases are uploaded here and never again.  The SRS handle is what the tier-1 hint kernels read Gamma1 through.
            self.dory_bases = bases  # the host arrays: what a verifier of this workload's proofs is set up with
            self.dory_setup = DoryProofSetup(ctx, bases["gamma1"], bases["gamma2"], bases["h1"], bases["h2"])
            self.srs = ctx.srs_upload(bases["gamma1"][:width])
            self.own_srs = True
            self.dory_commitment = None
            prng = np.random.default_rng(seed + 3)
            self.open_point = rand_fr(self.grid_vars, prng)
            self.column_of_claim = None  # the batch order is the caller's (final_opening_polynomial_order); None: the column order
            # the block-embedded polynomials are resident inputs like the witness columns: each its own balanced matrix (BlockOpeningPoly::new), columns after the dense ones
            from .dory_commit import block_sigma
            self.dory_blocks = [ctx.upload(b) for b in dory_blocks]
            self.dory_block_sigmas = [block_sigma(len(b)) for b in dory_blocks]
        elif pcs is not None:
            raise ValueError(pcs)
        self.tables, self.members, self.prepared, self.hint = {}, [], False, None
        self.prepare()
        ctx.synchronize()
        # input claims: in the real prover these are the previous stage's output claims; here computed once, untimed
        self.claims = [m.input_claim() for m in self.members]
        if pcs == "dory":
            # the statement of stage 8: every committed column's evaluation at the unified opening point, from one launch over the witness columns
            self.opening_claims = self.evaluate_columns()

    # ---- per-proof tables -------------------------------------------------------------------------------------------
    def _scale_table(self, spec):
        """eq(r_chunk, .) over the chunk domain (K entries) as host limbs (EqPolynomial::evals on the host: K = 16)"""
        return self.ffi.host_eq_evals(spec.point)

    def _make_table(self, name, spec):
        c = self.ctx
        if spec.kind == "onehot":  # dense address-folded column (only when a non-lazy member needs it)
            src = c.onehot(spec.data.reshape(1, -1), 1 << len(spec.point))
            st = c.eq_evals(spec.point)
            out = src.materialize(0, st)
            c.synchronize()
            st.free()
            src.free()
            return out
        if spec.kind in ("u64", "i64"):
            return c.table_from_ints(self.ints[name])
        if spec.kind == "eq":
            return c.eq_evals(spec.point)
        if spec.kind == "lt":
            return c.lt_evals(spec.point)
        if spec.kind == "eq1":
            eq, eq1 = c.eq_plus_one_evals(spec.point)
            eq.free()
            return eq1
        raise ValueError(spec.kind)

    def prepare(self):
        """Everything a proof builds before its first round: per-proof tables and the members over them."""
        if self.prepared:
            self.release()
        ctx = self.ctx
        for name, spec in self.tables_spec.items():
            if name not in self._skip:
                self.tables[name] = self._make_table(name, spec)
        for i, ms in enumerate(self.members_spec):
            if ms.uniform is not None:
                V, F, csyms = ms.uniform
                coeffs = [self.resolver.coeff(c) for c in csyms]
                w = self.tables_spec[ms.tables[0]].point
                if self._lazy(ms):
                    specs = [self.tables_spec[t] for t in ms.tables[1:]]
                    scale_tables = np.stack([self._scale_table(sp) for sp in specs])
                    m = ctx.member_lazy_ra_uniform(self.sources[i], scale_tables, V, F, coeffs, w)
                else:
                    tabs = [self.tables[t] for t in ms.tables[1:]]
                    m = ctx.member_split_eq_uniform(tabs, V, F, coeffs, w, borrow=True)
            elif ms.eq_inner is not None:
                dq, inner = ms.eq_inner
                m = ctx.member_lc([self._slot(t) for t in ms.tables[1:]], self.resolver.groups(inner), dq, borrow=True,
                                  eq_point=self.tables_spec[ms.tables[0]].point)
            elif ms.fused is not None:  # A = sum_i s_i * leaf_i as ONE table (jolt_rlc), then the ordinary member over fewer tables
                parts, names, groups = ms.fused
                for fname, entries in parts:
                    srcs = [self.tables[ms.tables[ti]] for _, ti in entries]
                    self.tables[fname] = ctx.rlc(srcs, np.stack([self.resolver.coeff(c) for c, _ in entries]))
                m = ctx.member_lc([self.tables[t] for t in names], self.resolver.groups(groups), ms.degree, borrow=True, skip_one=True)
            elif ms.split_eq is not None:
                a, b, w = ms.split_eq
                tabs = [self.tables[t] for t in ms.tables]
                m = ctx.member_split_eq_product(tabs[a], tabs[b], w, borrow=True)
            else:
                m = ctx.member_lc([self._slot(t) for t in ms.tables], self.resolver.groups(ms.groups), ms.degree, borrow=True, skip_one=True)
            self.members.append(m)
        self.prepared = True

    def _slot(self, name):
        """a member's table slot: the resident integer column for a compact-scalar witness column, the per-proof field table otherwise"""
        return self.ints[name] if name in self._small else self.tables[name]

    # ---- the witness path: packed rows -> one upload -> columns on the device ------------------------------------
    def pack_witness_rows(self):
        """(rows (T, row_bytes) uint8, layout): per cycle every integer witness column as 8 bytes, then per index-encoded member ONE address field whose nibbles are
        its RA chunks (the instruction lookup index: 16 bytes for 32 chunks; the RAM address: 2 bytes for 4) and a validity byte (0 = no access: cold cycle)"""
        T = 1 << self.n_vars
        names = list(self.ints)
        fields, off = [], 0
        for name in names:
            fields.append(("int", name, off, 8))
            off += 8
        for i in sorted(self.sources):
            ms = self.members_spec[i]
            n, log_k = len(ms.tables) - 1, len(self.tables_spec[ms.tables[1]].point)
            width = (n * log_k + 7) // 8
            assert width <= 16
            fields.append(("onehot", i, off, width, n, log_k))
            off += width + 1
        row_bytes = (off + 7) // 8 * 8
        rows = np.zeros((T, row_bytes), dtype=np.uint8)
        for f in fields:
            if f[0] == "int":
                spec = self.tables_spec[f[1]]
                col = spec.data.astype(np.uint64 if spec.kind == "u64" else np.int64).view(np.uint64)
                rows[:, f[2]:f[2] + 8] = col.reshape(-1, 1).view(np.uint8).reshape(T, 8)
            else:
                _, i, o, width, n, log_k = f
                cols = [self.tables_spec[t].data for t in self.members_spec[i].tables[1:]]
                hot = cols[0] != 0xFF
                assert all(np.array_equal(c != 0xFF, hot) for c in cols), "the chunks of one address are cold together"
                per = 8 // log_k  # chunks per byte
                for b in range(width):
                    byte = np.zeros(T, dtype=np.uint8)
                    for q in range(per):
                        k = b * per + q
                        if k < n:
                            byte |= (np.where(hot, cols[k], 0).astype(np.uint8) << np.uint8(q * log_k))
                    rows[:, o + b] = byte
                rows[:, o + width] = hot.astype(np.uint8)
        return rows, fields

    def upload_witness(self):
        """one step's witness from host memory: ONE copy of the packed rows, then device-side extraction into the columns the members read"""
        if getattr(self, "_packed", None) is None:
            rows, self._fields = self.pack_witness_rows()
            if self.witness_pinned:  # the tracer's row buffer in page-locked memory (jolt_host_pinned_alloc): the copy runs at the link rate
                self._pinned = self.ffi.PinnedBuffer(self.ctx, rows.shape)
                self._pinned.array[...] = rows
                self._packed = self._pinned.array
            else:
                self._packed = rows
        import os, time
        trace = os.environ.get("JOLT_TRACE_UPLOAD") == "1"
        marks = []

        def mark(what):
            if trace:
                self.ctx.synchronize()
                marks.append((what, time.perf_counter()))
        mark("start")
        if self.hint is not None:  # a hint nobody opened with: it reads the columns that are replaced below
            self.hint.free()
            self.hint = None
        if self.prepared:
            self.release()  # the members of the previous proof borrow the columns that are replaced here
        mark("release")
        if self.witness_overlapped:
            rows = self._rows_in_flight if self._rows_in_flight is not None else self.ffi.Rows.begin(self.ctx, self._packed)  # (the first proof has nothing ahead of it)
            self._rows_in_flight = None
            rows.wait()
        else:
            rows = self.ffi.Rows(self.ctx, self._packed)
        mark("rows ready")
        int_fields = [f for f in self._fields if f[0] == "int"]
        extracted = rows.ints_many([(off, width, self.tables_spec[name].kind == "i64") for _, name, off, width in int_fields])  # every integer column in one pass over the rows
        for (_, name, _, _), new in zip(int_fields, extracted):
            self.ints[name].free()
            self.ints[name] = new
        for f in self._fields:
            if f[0] == "int":
                continue
            else:
                _, i, off, width, n, log_k = f
                new = rows.onehot(off, width, [k * log_k for k in range(n)], log_k, valid_offset=off + width)
                self.sources[i].free()
                self.sources[i] = new
        mark("extracted")
        rows.free()
        mark("rows freed")
        if self.witness_overlapped:  # the next proof's witness starts moving now, under this proof's kernels
            self._rows_in_flight = self.ffi.Rows.begin(self.ctx, self._packed)
        mark("next begun")
        if trace:
            import sys
            print("[upload trace] " + ", ".join(f"{b[0]} {1e3 * (b[1] - a[1]):.2f}" for a, b in zip(marks, marks[1:])), file=sys.stderr)

    def witness_bytes_per_cycle(self):
        if getattr(self, "_packed", None) is None:
            self._packed, self._fields = self.pack_witness_rows()
        return int(self._packed.shape[1])

    def release(self):
        if getattr(self, "dory_commitment", None) is not None:  # pcs="dory": this proof's hints go with its tables
            self.dory_commitment.close()
            self.dory_commitment = None
        for m in self.members:
            m.destroy()
        self.members = []
        for t in self.tables.values():
            t.free()
        self.tables = {}
        self.prepared = False

    # ---- the proof ---------------------------------------------------------------------------------------------------
    def prove_stage(self, stage, label=0):
        idxs = self.stages[stage]
        ms = [self.members[i] for i in idxs]
        deg = max(m.degree for m in ms)
        return self.ctx.prove_batch(ms, [self.claims[i] for i in idxs], [self.batch_coeffs[i] for i in idxs], [0] * len(ms), self.n_vars, deg, label=label + stage,
                                    use_round_group=True)

    def prove(self, label=0):
        """Every stage's batched sumcheck, then rewind the members (they borrow their tables). Returns per-stage outputs."""
        if not self.prepared:
            self.prepare()
        outs = {stage: self.prove_stage(stage, label) for stage in sorted(self.stages)}
        for m in self.members:
            m.reset()
        return outs

    def prove_stages(self, label=0):
        """Stages 1 .. 7 in protocol order: per stage the stage operators (their own context, the worker thread) BESIDE the stage's batched sumcheck of the catalogue (this
        thread); both finish before the next stage starts.  -> (the operators' outputs, the catalogue's per-stage outputs), the same values as `ext.prove` and `prove`."""
        if not self.prepared:
            self.prepare()
        ext_out, outs = {}, {}
        n_slots = len(self._stage_slots)
        for stage in sorted(set(self.stages) | set(self.ext.STAGES)):
            pending = [self._stage_slots[slot % n_slots][0].submit(chain) for slot, chain in self.ext.stage_chains(stage, label)]  # (one slot: its chains queue up in order)
            try:
                if stage in self.stages:
                    outs[stage] = self.prove_stage(stage, label)
            finally:
                results = []
                for f in pending:  # every chain is waited for, also when one of them (or the catalogue's batch) raised
                    try:
                        results.append(f.result())
                    except Exception as e:  # noqa: BLE001 -- re-raised below
                        results.append(e)
            for r in results:
                if isinstance(r, Exception):
                    raise r
                ext_out.update(r)
        for m in self.members:
            m.reset()
        return ext_out, outs

    # ---- whole protocol stages as ONE batch each ------------------------------------------------------------------------------------------------------------
    # The reference proves a stage as one prove_batch (crates/jolt-sumcheck/src/prover.rs:193-362) over the relations its verifier lists per stage
    # (crates/jolt-verifier/src/stages/stage{2,3,4,5,6a,6b,7}/outputs.rs).  Every window starts at the relation's instance_point_offset:
    #   the default, batch_num_vars - rounds                    crates/jolt-verifier/src/stages/relations.rs:202-213
    #   stage 2, RAM RAF evaluation and RAM output check        stage2/mod.rs:25-49 (phase1_instance_point_offset: the window of the read-write leader + its phase-1
    #       rounds; with all log T cycle rounds in phase 1, as the RAM read-write operator here runs them, that is batch_num_vars - log K: stage2/ram_raf_evaluation.rs:98-100,
    #       stage2/ram_output_check.rs:133-135, and their tests instance_point_offset_spans_the_batch_tail)
    # so every window of stages 2 .. 7 ends with its batch.  (Offset 0 is overridden only by the advice / precommitted reductions, stage6b/committed_reduction_cycle_phase.rs:139
    # and stage7/*_address_phase.rs:96,107 -- relations that exist here neither as a member nor as an operator.)
    STAGE_BATCHES = {2: ("ram_read_write", "spartan_product", "instruction_claim_reduction", "ram_raf_evaluation", "ram_output_check"),
                     3: ("spartan_shift", "instruction_input", "registers_claim_reduction"),
                     4: ("registers_read_write", "ram_val_check"),
                     5: ("instruction_read_raf", "ram_ra_claim_reduction", "registers_val_evaluation"),
                     "6a": ("bytecode_read_raf_address", "booleanity_address"),
                     "6b": ("bytecode_read_raf_cycle", "booleanity_cycle", "ram_hamming_booleanity", "ram_ra_virtualization", "instruction_ra_virtualization", "inc_claim_reduction"),
                     7: ("hamming_weight",)}
    STAGE_BATCH_LABELS = {2: 2, 3: 3, 4: 4, 5: 5, "6a": 6, "6b": 16, 7: 7}  # the transcript of stage s is label + this

    def stage_batch_coefficient(self, name):
        """the batching coefficient of relation `name` in its stage's batch: a random field element per relation, fixed per workload"""
        if getattr(self, "_stage_batch_coeffs", None) is None:
            names = [n for key in (2, 3, 4, 5, "6a", "6b", 7) for n in self.STAGE_BATCHES[key]]
            self._stage_batch_coeffs = dict(zip(names, rand_fr(len(names), np.random.default_rng(self._seed + 5))))
        return self._stage_batch_coeffs[name]

    def prove_stage_batches(self, label=0, stages=(2, 3, 4, 5, 6, 7), grouped=True, challenge_mode=0):
        """Every protocol stage as ONE batched sumcheck on the MAIN context (needs extended=True): the stage's operators come from the catalogue of `self.ext`
        (DeviceExtended.operator / input_claim, over its resident inputs), the stage's catalogue members are wrapped (Context.stage_member: borrowed), and jolt_host_prove_batch_ops_grouped runs the batch under label +
        STAGE_BATCH_LABELS[stage] -- per round ONE round-group launch set over the wrapped members, the operators beside it.  stages: a subset of (2, 3, 4, 5, 6, 7); 6 is
        6a followed by 6b (6b starts from what 6a leaves).  grouped=False: the same batches under SequentialRounds (the same bytes); challenge_mode: as Context.prove_batch_ops.
        -> {stage: what prove_batch_ops returns + names, rounds, offsets, input_claims, coefficients, max_num_vars, max_degree, output_claims (per operator)}.
        The members are rewound afterwards: `prove` / `step` see them as `prepare` left them."""
        if self.ext is None:
            raise ValueError("prove_stage_batches needs the stage operators' resident inputs: DeviceWorkload(..., extended=True)")
        if not self.prepared:
            self.prepare()
        ctx, ext = self.ctx, self.ext
        by_name = {ms.name: i for i, ms in enumerate(self.members_spec)}
        outs = {}

        def release(named):
            for _, op in reversed(named):  # (the bytecode cycle operator before the address operator it was prepared from)
                op.destroy()

        def run(key, claim=None, **given):
            """the batch of STAGE_BATCHES[key], the reference's order: a catalogue member wrapped, anything else an operator of ext.OPERATORS created with the arguments given[name]
            and proved under ext.input_claim (claim: booleanity's cycle phase's).  -> [(name, operator)], for the caller to read and release"""
            named = []
            try:
                for name in self.STAGE_BATCHES[key]:
                    named.append((name, ctx.stage_member(self.members[by_name[name]]) if name in by_name else ext.operator(name, ctx, **given.get(name, {}))))
                ops = [op for _, op in named]
                rounds = [op.rounds for op in ops]
                total, degree = max(rounds), max(op.degree for op in ops)
                offsets = [total - r for r in rounds]  # instance_point_offset (relations.rs:202-213; stage2/mod.rs:25-49): every window ends with the batch
                input_claims = [self.claims[by_name[name]] if name in by_name else ext.input_claim(name, op, claim) for name, op in named]
                coeffs = [self.stage_batch_coefficient(name) for name, _ in named]
                prove = ctx.prove_batch_ops_grouped if grouped else ctx.prove_batch_ops
                out = prove(ops, input_claims, coeffs, offsets, total, degree, label=label + self.STAGE_BATCH_LABELS[key], challenge_mode=challenge_mode)
                out.update(names=[name for name, _ in named], rounds=rounds, offsets=offsets, input_claims=[np.array(c, copy=True) for c in input_claims], coefficients=coeffs,
                           max_num_vars=total, max_degree=degree, output_claims=[op.output_claims() for op in ops])
                outs[key] = out
            except Exception:
                release(named)
                raise
            return named

        try:
            for stage in stages:
                if stage == 2:  # one index of the RAM address column for the stage
                    index = ext.ram_index(ctx)
                    try:
                        release(run(2, ram_raf_evaluation=dict(index=index), ram_output_check=dict(index=index)))
                    finally:
                        index.free()
                elif stage in (3, 4, 5, 7):
                    release(run(stage))
                elif stage == 6:  # 6b starts from what 6a leaves: the bound bytecode address operator, booleanity's window of the challenges and its intermediate claim
                    index = ext.pc_index(ctx)
                    try:
                        a_named = run("6a", bytecode_read_raf_address=dict(index=index))
                        try:
                            a, k = outs["6a"], self.STAGE_BATCHES["6a"].index("booleanity_address")
                            r_address = a["challenges"][a["offsets"][k]:][::-1]  # most significant address bit first
                            b_named = run("6b", claim=a["output_claims"][k][0], bytecode_read_raf_cycle=dict(address=dict(a_named)["bytecode_read_raf_address"]),
                                          booleanity_cycle=dict(r_address=r_address))
                            outs["6b"]["eq_scalar"] = dict(b_named)["booleanity_cycle"].kept("eq_scalar")[0]
                            release(b_named)
                        finally:
                            release(a_named)
                    finally:
                        index.free()
                else:
                    raise ValueError(f"no stage batch {stage!r}")
        finally:
            for m in self.members:  # the wrapped members were borrowed: back to round 0 for the next prove / step
                m.reset()
        return outs

    def commit(self):
        """Stage 0 over the commitment grid: dense increment columns = T-term MSMs of 64-bit scalars against the SRS prefix (address 0),
        one-hot columns = sums of selected bases.  pcs="dory": dory_commit."""
        if self.pcs == "dory":
            return self.dory_commit()
        ctx, T = self.ctx, 1 << self.n_vars
        # the dense columns' MSMs go in flight on the side lanes (short: bound by the latency of their sort and reduction chains) and are collected after the one-hot
        # sums of bases have run on the main stream (bound by multiplications); a context that cannot hold them in flight: one after the other
        pending = None
        if self.committed_dense:
            try:
                pending = ctx.msm_tables_begin(self.srs, [self.tables[name] for name in self.committed_dense], [T] * len(self.committed_dense))
            except self.ffi.JoltError as e:
                if e.status != 6:  # JOLT_ERR_UNSUPPORTED: this context cannot hold them in flight
                    raise
        dense = None if pending is not None else [ctx.msm(self.srs, self.tables[name], T) for name in self.committed_dense]
        try:
            onehot = [ctx.grid_commit_onehot(self.srs, self.sources[i]) for i in sorted(self.sources)]
        finally:
            if pending is not None:
                dense = list(pending.finish())
        # the opening hint (CommitmentScheme::commit returns (Commitment, OpeningHint), schemes.rs:60-72): the class sums behind the opening's first level commitments are a
        # function of the witness and the SRS alone -- enqueued now in the background, they run under the latency-bound stage operators and sumcheck legs
        levels = self.linear_levels()
        if levels:
            if self.hint is not None:
                self.hint.free()
            self.hint = ctx.grid_hint(self.srs, [self.sources[i] for i in sorted(self.sources)], levels, background=True)
        return dict(dense=np.stack(dense), onehot=np.concatenate(onehot))

    def joint_polynomial(self):
        return self.ctx.grid_joint_polynomial([self.sources[i] for i in sorted(self.sources)], self.rlc_onehot,
                                              [self.tables[name] for name in self.committed_dense], self.rlc_dense, self.log_k)

    def linear_levels(self):
        """how many of the opening's first level commitments come by linearity from the commit-time hint: 2 (three cost +13 ms, profiles/r04_open_linear_levels_ab.txt), fewer on small grids"""
        return max(0, min(2, self.grid_vars - 1, self.n_vars - 1))

    def open(self, label=0):
        """Stage 8: joint polynomial of the homomorphic batch, one HyperKZG opening at the unified point; the first level commitments by linearity from the opening hint
        the commit leg left in flight (jolt_host_hyperkzg_open_grid) -- begun here if this proof has none.  pcs="dory": dory_open."""
        if self.pcs == "dory":
            return self.dory_open(label)
        joint = self.joint_polynomial()
        levels = self.linear_levels()
        if levels and self.hint is None:
            self.hint = self.ctx.grid_hint(self.srs, [self.sources[i] for i in sorted(self.sources)], levels, background=False)
        if levels:
            out = self.ctx.hyperkzg_open_grid(self.srs, joint, self.open_point, self.hint, levels, self.rlc_onehot, [self.tables[name] for name in self.committed_dense],
                                              self.rlc_dense, label=label)
        else:
            out = self.ctx.hyperkzg_open(self.srs, joint, self.open_point, label=label)
        if self.hint is not None:
            self.hint.free()
            self.hint = None
        joint.free()
        return out

    # ---- pcs="dory": the same columns under the reference's production scheme ------------------------------------------------------------------------------
    @staticmethod
    def _check_dory_shape(n_vars, seed, blocks, order, log_extra, log_k=4):
        """the refusals of pcs="dory" that need no device: the placement, and every block against the grid of 2^nu x 2^sigma.  -> the blocks as host arrays (an int m
        becomes 2^m field elements drawn from the seed)"""
        if order not in ("cycle_major", "address_major"):
            raise ValueError("dory_order is cycle_major or address_major")
        if log_extra < 0 or (log_extra and order != "address_major"):
            raise ValueError("dory_log_extra widens the address-major grid only")
        grid_vars = log_k + n_vars + log_extra
        sigma = (grid_vars + 1) // 2
        nu = grid_vars - sigma
        if order == "address_major" and sigma < log_k + log_extra:
            raise ValueError("address_major: sigma < log_k + log_extra, a cycle's block is wider than a matrix row")
        if len(blocks) > 256:
            raise ValueError("at most 256 blocks")
        rng = np.random.default_rng(seed + 4)
        out = []
        for b in blocks:
            if isinstance(b, (int, np.integer)):
                if not 0 <= b <= grid_vars:
                    raise ValueError("a block does not fit the grid")
                b = rand_fr(1 << int(b), rng)
            b = np.ascontiguousarray(b, dtype=np.uint64).reshape(-1, 4)
            n = b.shape[0]
            if n == 0 or n & (n - 1):
                raise ValueError("a block holds a power of two of field elements")
            sigma_p = (n.bit_length() - 1 + 1) // 2  # dory_commit.block_sigma
            if sigma_p > sigma or n >> sigma_p > 1 << nu:
                raise ValueError("a block does not fit the grid")
            out.append(b)
        return out

    def _dory_columns(self):
        """(sources, dense field tables): the joint polynomial's columns in jolt_dory_fold_rows_grid's order"""
        return [self.sources[i] for i in sorted(self.sources)], [self.tables[name] for name in self.committed_dense]

    def evaluate_columns(self):
        """(columns, 4): every committed column's evaluation at open_point, ONE launch over the witness columns (jolt_grid_evaluate_columns), then the blocks' claims
        from one launch over the blocks (jolt_dory_evaluate_blocks).  open_point is in grid order: address then cycle coordinates cycle-major; cycle, address, extra
        coordinates address-major -- the same column at the permuted point, times the Lagrange factor prod (1 - e) of the extra coordinates at zero."""
        if not self.prepared:
            self.prepare()
        sources, dense = self._dory_columns()
        if getattr(self, "dory_order", "cycle_major") == "address_major":
            ffi, n, k = self.ffi, self.n_vars, self.log_k
            cycle, address, extra = self.open_point[:n], self.open_point[n:n + k], self.open_point[n + k:]
            claims = self.ctx.grid_evaluate_columns(sources, dense, k, np.concatenate([address, cycle]))
            if len(extra):
                scale = self.one
                for e in extra:
                    scale = ffi.host_fr_mul(scale, ffi.host_fr_sub(self.one, e))
                claims = np.stack([ffi.host_fr_mul(c, scale) for c in claims])
        else:
            claims = self.ctx.grid_evaluate_columns(sources, dense, self.log_k, self.open_point)
        if getattr(self, "dory_blocks", None):
            claims = np.concatenate([claims, self.ctx.dory_evaluate_blocks(self.dory_blocks, self.dory_block_sigmas, self.open_point, self.dory_sigma)])
        return claims

    def evaluate_columns_pushforward(self):
        """the same claims by the route that preceded that entry, kept as the second implementation the tests hold it against: per source one
        jolt_onehot_pushforward of the cycles' eq table, its K-entry masses downloaded and dotted with the addresses' eq table on the host; a dense column is
        eq_a[0] * <eq_c, column>"""
        if not self.prepared:
            self.prepare()
        ffi, ctx = self.ffi, self.ctx
        sources, dense = self._dory_columns()
        eq_a = ffi.host_eq_evals(self.open_point[:self.log_k])
        eq_c = ctx.eq_evals(self.open_point[self.log_k:])
        out = []
        try:
            for s in sources:
                masses = s.pushforward(eq_c)
                g = masses.download().reshape(s.n_polys, s.k, 4)
                masses.free()
                out += [ffi.host_fr_wide_dot(g[p], eq_a[:s.k]) for p in range(s.n_polys)]
            for t in dense:
                out.append(ffi.host_fr_mul(ctx.table_dot(t, eq_c), eq_a[0]))
        finally:
            eq_c.free()
        return np.stack(out)

    def dory_commit(self):
        """Stage 0 under Dory: tier 1 into resident hints (one jolt_dory_hints_onehot per source, one jolt_dory_hints_rows per integer column), tier 2 as ONE product
        batch against the setup's prepared Gamma2.  The commitment object stays as this proof's opening hint.  -> dict(tier2=(columns, 48))"""
        from .dory_commit import DoryWitnessCommitment
        if self.dory_commitment is not None:  # a hint nobody released
            self.dory_commitment.close()
            self.dory_commitment = None
        sources = [self.sources[i] for i in sorted(self.sources)]
        self.dory_commitment = DoryWitnessCommitment(self.dory_setup, self.srs, sources, [self.ints[name] for name in self.committed_dense], self.dory_sigma,
                                                     order=self.dory_order, log_k=self.log_k, log_extra=self.dory_log_extra, blocks=self.dory_blocks)
        return dict(tier2=np.stack(self.dory_setup.tier2(self.dory_commitment.hints)))

    def dory_open(self, label=0, evaluations=None, column_of_claim=None):
        """Stage 8 under Dory: HomomorphicBatch::prove_batch as ONE call of the library (jolt_host_dory_prove_batch) under a transcript of the label's engine -- the
        statement, gamma's powers, the row fold, the check <v, R> == joint_eval, the evaluation proof, the closing claim.  evaluations / column_of_claim: the
        statement's claims and their batch order (default: opening_claims in self.column_of_claim's order; claim i is column column_of_claim[i]).
        -> what Context.dory_prove_batch returns + transcript_state (32 bytes, after the closing claim)"""
        if self.dory_commitment is None:
            self.dory_commit()
        order = self.column_of_claim if column_of_claim is None else column_of_claim
        hints = self.dory_commitment.hints if order is None else [self.dory_commitment.hints[c] for c in order]
        if evaluations is None:
            evaluations = self.opening_claims if order is None else self.opening_claims[list(order)]
        sources, dense = self._dory_columns()
        transcript = self.ffi.HostTranscript(label)
        try:
            out = self.ctx.dory_prove_batch(self.dory_setup, hints, evaluations, sources, dense, self.log_k, self.open_point, transcript, column_of_claim=order,
                                            blocks=self.dory_blocks, block_sigmas=self.dory_block_sigmas, order=self.dory_order, log_extra=self.dory_log_extra)
            out["transcript_state"] = transcript.state()
        finally:
            transcript.close()
        return out

    def dory_verify(self, commit_out, open_out, label=0, evaluations=None):
        """The verifier of stage 8 under Dory: HomomorphicBatch::verify_batch as ONE call of the library (jolt_host_dory_verify_batch) under a fresh transcript of the
        label's engine.  commit_out: what dory_commit returned (its tier2 array, in column order); open_out: what dory_open returned; the statement is opening_claims
        (or `evaluations`, in batch order) at open_point.  A verifier sees neither the placement nor the blocks.  -> bool; the details of the last call -- accepted,
        failed_check, joint_eval, transcript_state (equal to dory_open's after an accepted proof) -- stay in self.dory_verify_result."""
        order = self.column_of_claim
        tier2 = np.asarray(commit_out["tier2"], dtype=np.uint64).reshape(-1, 48)
        commitments = tier2 if order is None else tier2[list(order)]
        if evaluations is None:
            evaluations = self.opening_claims if order is None else self.opening_claims[list(order)]
        transcript = self.ffi.HostTranscript(label)
        try:
            out = self.ctx.dory_verify_batch(self.dory_setup.verifier(), commitments, evaluations, self.open_point, open_out, transcript)
            out["transcript_state"] = transcript.state()
        finally:
            transcript.close()
        self.dory_verify_result = out
        return out["accepted"]

    def verify(self, commit_out, open_out, label=0, evaluations=None):
        """The verifier of stage 8 under HyperKZG (pcs="grid"), the counterpart of dory_verify: the step's own opening as the step frames it, ONE call of the library
        (jolt_host_hyperkzg_verify) under a fresh transcript of the label's engine.  commit_out: what commit() returned; its commitments enter in the joint
        polynomial's column order (one-hot source by source, then dense) under rlc_onehot / rlc_dense -- verify after combine, C_0 never built; open_out: what open()
        returned; the joint evaluation is formed from evaluate_columns() (or `evaluations`, in that column order) and the same scalars, at open_point.  The verifier
        setup comes from the workload's own test secret on first use and is kept.  -> bool; the details of the last call -- accepted, failed_check, failed_level,
        joint_eval, transcript_state -- stay in self.verify_result.  step() does not call it."""
        if self.pcs != "grid":
            raise ValueError('verify is the verifier of pcs="grid"; pcs="dory" has dory_verify')
        ffi = self.ffi
        if getattr(self, "verifier_setup", None) is None:
            if getattr(self, "beta", None) is None:
                raise ValueError("a workload over a caller's SRS does not know its secret: build a HyperKzgVerifierSetup from the setup's G2 points")
            from .dory_setup import g2_generator
            self.verifier_setup = self.ctx.hyperkzg_verifier_setup(G1_GENERATOR, g2_generator(), beta=self.beta)
        commitments = np.concatenate([np.asarray(commit_out["onehot"], dtype=np.uint64).reshape(-1, 12), np.asarray(commit_out["dense"], dtype=np.uint64).reshape(-1, 12)])
        scalars = np.concatenate([self.rlc_onehot.reshape(-1, 4), self.rlc_dense.reshape(-1, 4)])
        if evaluations is None:
            evaluations = self.evaluate_columns()
        evaluations = np.asarray(evaluations, dtype=np.uint64).reshape(-1, 4)
        if evaluations.shape[0] != scalars.shape[0] or commitments.shape[0] != scalars.shape[0]:
            raise ValueError("one commitment and one evaluation per column")
        joint = np.zeros(4, dtype=np.uint64)
        for s, y in zip(scalars, evaluations):
            joint = ffi.host_fr_add(joint, ffi.host_fr_mul(s, y))
        transcript = ffi.HostTranscript(label)
        try:
            out = self.ctx.hyperkzg_verify(self.verifier_setup, commitments, self.open_point, joint, open_out, transcript=transcript, commitment_scalars=scalars)
            out["transcript_state"] = transcript.state()
        finally:
            transcript.close()
        out["joint_eval"] = joint
        self.verify_result = out
        return out["accepted"]

    def step(self, label=0):
        """One proof's worth of hot-path work (bench.py's timed step)."""
        if self.witness_upload:
            self.upload_witness()
        self.prepare()
        out = {}
        if self.pcs:
            out["commit"] = self.commit()
        if self.ext is not None and self._stage_worker is not None:
            out["extended"], out["stages"] = self.prove_stages(label)
        else:
            if self.ext is not None:
                out["extended"] = self.ext.prove(label)
            out["stages"] = self.prove(label)
        if self.pcs:
            out["open"] = self.open(label)
        return out

    def bytes_resident(self):
        return sum(len(t) for t in self.tables.values()) * 32

    def close(self):
        if getattr(self, "hint", None) is not None:  # (before the sources it reads)
            self.hint.free()
            self.hint = None
        self.release()
        if self.ext is not None:
            self.ext.close()
            self.ext = None
        for pool, slot_ctx in self._stage_slots:
            pool.shutdown(wait=True)
            if slot_ctx is not self.ext_ctx:
                slot_ctx.close()
        self._stage_slots, self._stage_worker = [], None
        if self.ext_ctx is not None:
            self.ext_ctx.close()
            self.ext_ctx = None
        for s in self.sources.values():
            s.free()
        for v in self.ints.values():
            v.free()
        self.sources, self.ints = {}, {}
        for b in getattr(self, "dory_blocks", []):
            b.free()
        self.dory_blocks = []
        if getattr(self, "_rows_in_flight", None) is not None:
            self._rows_in_flight.free()
            self._rows_in_flight = None
        if getattr(self, "_pinned", None) is not None:
            self._packed = None
            self._pinned.free()
            self._pinned = None
        if self.own_srs and self.srs is not None:
            self.srs.free()
            self.srs = None
        if getattr(self, "dory_setup", None) is not None:
            self.dory_setup.close()
            self.dory_setup = None
        if getattr(self, "verifier_setup", None) is not None:
            self.verifier_setup.close()
            self.verifier_setup = None


# BN254 G1 generator (1, 2) as Montgomery Jacobian limbs (ark_bn254::G1Projective layout): R mod q, 2R mod q, R mod q
_Q = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47


def _fq_mont(v):
    m = (v << 256) % _Q
    return [(m >> (64 * i)) & (2**64 - 1) for i in range(4)]


G1_GENERATOR = np.array(_fq_mont(1) + _fq_mont(2) + _fq_mont(1), dtype=np.uint64)
