#!/usr/bin/env python3
"""Generate rust/jolt-kernels-hip/src/ffi.rs from include/jolt_hip.h as jolt_amd/abi.py reads it (and parse either side for the agreement test).

The image has no Rust toolchain, so the FFI crate cannot be compiled here; what CAN be guaranteed mechanically is that the Rust
declarations name every entry point of the C header with the same arity and the same types.  tests/test_abi_cpu.py re-parses both
files with the functions below and compares them declaration by declaration.

    python tools/gen_rust_ffi.py            # rewrite ffi.rs
    python tools/gen_rust_ffi.py --check    # exit 1 if ffi.rs is stale
"""
import os
import re
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
FFI_RS = os.path.join(ROOT, "rust", "jolt-kernels-hip", "src", "ffi.rs")

sys.path.insert(0, ROOT)
from jolt_amd import abi  # noqa: E402  (the header's parser lives with the Python binding, which reads the same declarations)

SCALARS = {"int32_t": "i32", "uint32_t": "u32", "uint64_t": "u64", "int64_t": "i64", "uint8_t": "u8", "uint16_t": "u16", "size_t": "usize", "float": "f32", "double": "f64",
           "void": "c_void", "char": "c_char"}


def c_type_to_rust(ctype):
    """('jolt_fr_t', (True, True)), i.e. 'const jolt_fr_t *const *' -> '*const *const jolt_fr_t' (pointer levels read right to left)."""
    base, consts = ctype
    rust = SCALARS.get(base, base)
    for const in consts:
        rust = ("*const " if const else "*mut ") + rust
    return rust


def parse_header(path=abi.HEADER):
    """-> list of (name, ret_rust, [(param_name, rust_type)]) in declaration order"""
    return [(name, c_type_to_rust(ret), [(p, c_type_to_rust(t)) for p, t in params]) for name, ret, params in abi.parse_header(path)]


def parse_rust(path=FFI_RS):
    src = re.sub(r"//.*", "", open(path).read())
    decls = []
    for m in re.finditer(r"pub fn (jolt_\w+)\s*\((.*?)\)\s*(?:->\s*([^;]+))?;", src, flags=re.S):
        name, params, ret = m.group(1), " ".join(m.group(2).split()), (m.group(3) or "()").strip()
        plist = []
        if params:
            for p in re.split(r",\s*(?=(?:r#)?\w+\s*:)", params.rstrip(", ")):
                pname, ptype = p.split(":", 1)
                plist.append((pname.strip(), ptype.strip()))
        decls.append((name, ret, plist))
    return decls


RUST_KEYWORDS = {"type", "ref", "box", "in", "fn", "loop", "match", "move", "self", "where", "use", "mod", "impl", "struct", "enum"}


def render(decls):
    out = []
    out.append("//! Raw FFI declarations of `libjolt_hip.so` -- GENERATED from `include/jolt_hip.h` by `tools/gen_rust_ffi.py`; do not edit.")
    out.append("//! One declaration per entry point of the C header, same order, same arity, same types (checked by tests/test_abi_cpu.py).")
    out.append("//! `jolt_fr_t` is bit-identical to `jolt_field::Fr` (4 x u64 Montgomery limbs, crates/jolt-field/src/bn254/mod.rs:33-43) and")
    out.append("//! `jolt_g1_t` to `jolt_crypto::Bn254G1` (ark_bn254::G1Projective, crates/jolt-crypto/src/ec/bn254/mod.rs:17-24); `jolt_g2_t` to ark_bn254::G2Projective, `jolt_gt_t` to ark_bn254::Fq12 (Bn254GT).")
    out.append("#![allow(non_camel_case_types, clippy::too_many_arguments, clippy::missing_safety_doc)]")
    out.append("use core::ffi::{c_char, c_void};")
    out.append("")
    out.append("pub const JOLT_HIP_ABI_VERSION: i32 = 1;")
    out.append("")
    out.append("#[repr(C)]\n#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]\npub struct jolt_fr_t {\n    pub l: [u64; 4],\n}")
    out.append("#[repr(C)]\n#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]\npub struct jolt_fq_t {\n    pub l: [u64; 4],\n}")
    out.append("#[repr(C)]\n#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]\npub struct jolt_g1_t {\n    pub x: jolt_fq_t,\n    pub y: jolt_fq_t,\n    pub z: jolt_fq_t,\n}")
    out.append("#[repr(C)]\n#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]\npub struct jolt_fq2_t {\n    pub c0: jolt_fq_t,\n    pub c1: jolt_fq_t,\n}")
    out.append("#[repr(C)]\n#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]\npub struct jolt_g2_t {\n    pub x: jolt_fq2_t,\n    pub y: jolt_fq2_t,\n    pub z: jolt_fq2_t,\n}")
    out.append("#[repr(C)]\n#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]\npub struct jolt_gt_t {\n    pub c: [jolt_fq_t; 12],\n}")
    for o in abi.opaque_handles():
        out.append(f"#[repr(C)]\npub struct {o} {{\n    _private: [u8; 0],\n}}")
    out.append("")
    out.append("/// Status codes (`enum` of the header); see `crate::status` for the mapping onto the reference's error types.")
    for k, name in enumerate(["JOLT_OK", "JOLT_ERR_INVALID_ARG", "JOLT_ERR_NO_DEVICE", "JOLT_ERR_OOM", "JOLT_ERR_HIP", "JOLT_ERR_SIZE_MISMATCH", "JOLT_ERR_UNSUPPORTED",
                              "JOLT_ERR_NOT_FULLY_BOUND", "JOLT_ERR_ROUND_CHECK", "JOLT_ERR_SRS_TOO_SMALL", "JOLT_ERR_EMPTY_POINT", "JOLT_ERR_NOT_INVERTIBLE"]):
        out.append(f"pub const {name}: i32 = {k};")
    out.append("pub const JOLT_ORDER_LOW_TO_HIGH: i32 = 0;\npub const JOLT_ORDER_HIGH_TO_LOW: i32 = 1;")
    out.append("pub const JOLT_TRACE_CYCLE_MAJOR: i32 = 0;\npub const JOLT_TRACE_ADDRESS_MAJOR: i32 = 1;")
    out.append("pub const JOLT_MEMBER_FLAG_SKIP_ONE: u32 = 1;\npub const JOLT_MEMBER_FLAG_BORROW_TABLES: u32 = 2;")
    out.append("pub const JOLT_INT_U64: i32 = 0;\npub const JOLT_INT_I64: i32 = 1;\npub const JOLT_INT_I128: i32 = 2;\npub const JOLT_SCALAR_FR: i32 = 3;")
    out.append("pub const JOLT_FQ2_ADD: i32 = 0;\npub const JOLT_FQ2_SUB: i32 = 1;\npub const JOLT_FQ2_MUL: i32 = 2;\npub const JOLT_FQ2_SQR: i32 = 3;\npub const JOLT_FQ2_NEG: i32 = 4;")
    out.append("pub const JOLT_FQ12_MUL: i32 = 0;\npub const JOLT_FQ12_SQR: i32 = 1;\npub const JOLT_FQ12_INV: i32 = 2;\npub const JOLT_FQ12_CONJ: i32 = 3;\npub const JOLT_FQ12_FROBENIUS1: i32 = 4;\n"
               "pub const JOLT_FQ12_FROBENIUS2: i32 = 5;\npub const JOLT_FQ12_FROBENIUS3: i32 = 6;\npub const JOLT_FQ12_MUL_SPARSE: i32 = 7;\npub const JOLT_PAIRING_LINES: usize = 88;")
    out.append("pub const JOLT_DORY_KIND_G1: i32 = 0;\npub const JOLT_DORY_KIND_G2: i32 = 1;\npub const JOLT_DORY_KIND_FR: i32 = 2;\n"
               "pub const JOLT_DORY_PAIR: i32 = 0;\npub const JOLT_DORY_MSM_G1: i32 = 1;\npub const JOLT_DORY_MSM_G2: i32 = 2;")
    out.append("pub const JOLT_DORY_UPDATE_BETA: i32 = 0;\npub const JOLT_DORY_UPDATE_ALPHA: i32 = 1;\n"
               "pub const JOLT_DORY_PHASE_VMV: i32 = 0;\npub const JOLT_DORY_PHASE_FIRST: i32 = 1;\npub const JOLT_DORY_PHASE_SECOND: i32 = 2;\n"
               "pub const JOLT_DORY_PHASE_GAMMA: i32 = 3;\npub const JOLT_DORY_PHASE_FINAL: i32 = 4;")
    out.append("pub const JOLT_ROUND_PATH_TAIL: usize = 0;\npub const JOLT_ROUND_PATH_GROUP: usize = 1;\npub const JOLT_ROUND_PATH_SMALL: usize = 9;\n"
               "pub const JOLT_ROUND_PATH_SPLIT_EQ_PRODUCT: usize = 10;\npub const JOLT_ROUND_PATH_UNIFORM_ITEMS: usize = 12;\npub const JOLT_ROUND_PATH_UNIFORM_ROWS: usize = 13;\n"
               "pub const JOLT_ROUND_PATH_LAZY: usize = 14;\npub const JOLT_ROUND_PATH_BIND: usize = 15;\npub const JOLT_ROUND_PATH_COUNT: usize = 17;")
    out.append("".join(f"pub const JOLT_FX_PLAN_{name}: usize = {k};\n" for k, name in enumerate(
        ["C", "W", "LO_BITS", "SOA", "WIDE", "CAPACITY", "TWO_PASS", "GRID_REDUCE", "HEAVY_THRESHOLD", "STAGE_CAP", "NB1", "MAX_LDS", "OVERFLOW", "LARGEST_SEGMENT",
         "HEAVY_SEGMENTS", "WORDS"])) + "pub const JOLT_FX_PLAN_STALE: u32 = u32::MAX;")
    out.append("pub const JOLT_MAX_MEMBER_TABLES: usize = 40;\npub const JOLT_MAX_MEMBER_TERMS: usize = 16;\npub const JOLT_MAX_MEMBER_FACTORS: usize = 64;\npub const JOLT_MAX_DEGREE: usize = 7;")
    out.append("")
    out.append("#[repr(C)]\npub struct jolt_member_desc {\n    pub n_tables: u32,\n    pub n_terms: u32,\n    pub degree: u32,\n    pub order: i32,\n"
               "    pub term_offsets: *const u32,\n    pub factors: *const u32,\n    pub coeffs: *const jolt_fr_t,\n}")
    out.append("#[repr(C)]\npub struct jolt_member_lc_desc {\n    pub n_tables: u32,\n    pub n_groups: u32,\n    pub n_factors: u32,\n    pub n_lc: u32,\n    pub degree: u32,\n"
               "    pub order: i32,\n    pub flags: u32,\n    pub group_factor_offsets: *const u32,\n    pub factor_lc_offsets: *const u32,\n    pub factor_consts: *const jolt_fr_t,\n"
               "    pub lc_tables: *const u32,\n    pub lc_coeffs: *const jolt_fr_t,\n}")
    out.append("#[repr(C)]\npub struct jolt_dory_item {\n    pub op: i32,\n    pub a: *const jolt_dory_vec,\n    pub a_first: usize,\n    pub b: *const jolt_dory_vec,\n    pub b_first: usize,\n"
               "    pub prepared: *const jolt_g2_prepared,\n    pub prepared_first: usize,\n    pub n: usize,\n}")
    out.append("#[repr(C)]\n#[derive(Clone, Copy)]\npub struct jolt_dory_result {\n    pub w: [u64; 48],\n}")
    out.append("pub type jolt_local_round_fn = Option<\n    unsafe extern \"C\" fn(user: *mut c_void, active: *const usize, n_active: usize, binds: *const *const jolt_fr_t, evals_out: *mut jolt_fr_t, evals_count: usize) -> i32,\n>;")
    out.append("pub type jolt_gather_fn = Option<unsafe extern \"C\" fn(user: *mut c_void, local: *const jolt_fr_t, count: usize, gathered: *mut jolt_fr_t) -> i32>;")
    out.append("pub type jolt_round_transcript_fn = Option<unsafe extern \"C\" fn(user: *mut c_void, compressed_coeffs: *const jolt_fr_t, n_coeffs: usize, challenge_out: *mut jolt_fr_t) -> i32>;")
    out.append("pub type jolt_open_transcript_fn = Option<\n    unsafe extern \"C\" fn(user: *mut c_void, phase: i32, points: *const jolt_g1_t, n_points: usize, values: *const jolt_fr_t, n_values: usize, challenge_out: *mut jolt_fr_t) -> i32,\n>;")
    out.append("pub type jolt_dory_transcript_fn = Option<\n    unsafe extern \"C\" fn(user: *mut c_void, phase: i32, round: usize, gts: *const jolt_gt_t, n_gt: usize, g1s: *const jolt_g1_t, n_g1: usize, "
               "g2s: *const jolt_g2_t, n_g2: usize, challenge_out: *mut jolt_fr_t) -> i32,\n>;")
    out.append("")
    out.append('#[link(name = "jolt_hip")]\nextern "C" {')
    for name, ret, params in decls:
        ps = ", ".join(f"{('r#' + p) if p in RUST_KEYWORDS else p}: {t}" for p, t in params)
        out.append(f"    pub fn {name}({ps})" + (f" -> {ret};" if ret != "c_void" else ";"))
    out.append("}")
    return "\n".join(out) + "\n"


def main():
    text = render(parse_header())
    if "--check" in sys.argv:
        sys.exit(0 if os.path.exists(FFI_RS) and open(FFI_RS).read() == text else 1)
    os.makedirs(os.path.dirname(FFI_RS), exist_ok=True)
    open(FFI_RS, "w").write(text)
    print(f"{FFI_RS}: {len(parse_header())} entry points")


if __name__ == "__main__":
    main()
