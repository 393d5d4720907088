"""Measurement-only variants of the product kernels, kept OUT of the product source: each variant is
a set of textual patches applied to a temporary copy of inr-for-audio_amd/csrc, compiled to
inr-for-audio_amd/libsiren_<name>.so (never loaded by the package; tools/ab_bench.py times it
beside the product library in one process and checks bit-identity).

    python tools/variants.py st_nt stsc1     # build
    python tools/ab_bench.py --libs base=inr-for-audio_amd/libsiren_hip.so,st_nt=inr-for-audio_amd/libsiren_st_nt.so
    python tools/variants.py --check         # every variant's patches still apply (text only)

A variant whose patch targets a kernel edit removed is deleted here; its result stays in profiles/.
"""
from __future__ import annotations

import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "inr-for-audio_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "inr-for-audio_amd"))
from buildinfo import SOURCES  # noqa: E402  (the product library's source list)

_ST16 = "__device__ __forceinline__ void st16(h16* dst, uint4 v) { *(uint4*)dst = v; }"


def _st16_asm(pol: str) -> str:
    # the asm store carries its own s_nop: a VALU write of the data VGPRs must wait a cycle after a
    # 128-bit store, which hipcc's hazard recognizer does not see inside inline asm
    return ("__device__ __forceinline__ void st16(h16* dst, uint4 v) {\n"
            "  typedef unsigned u32x4 __attribute__((ext_vector_type(4)));\n"
            "  const u32x4 w = u32x4{v.x, v.y, v.z, v.w};\n"
            f"  asm volatile(\"global_store_dwordx4 %0, %1, off {pol}\\n\\ts_nop 1\" ::\"v\"(dst), \"v\"(w) : \"memory\");\n"
            "}")


# forward epilogue stores through buffer descriptors of the wave's 128-row band (base in SGPRs,
# one 32-bit lane offset, the row subtile in soffset) instead of 64-bit per-lane addresses
_BST_OLD1 = """  float hp[SM];
#pragma unroll
  for (int j = 0; j < SM; ++j) hp[j] = 0.f;"""
_BST_NEW1 = """  float hp[SM];
#pragma unroll
  for (int j = 0; j < SM; ++j) hp[j] = 0.f;
  const int N = p.N;
  const size_t obase = (size_t)(m0 + w.wm * TM) * N + n0;
  const auto rsy = __builtin_amdgcn_make_buffer_rsrc(p.Y + obase, (short)0, TM * N * 2, 0x00020000);
  const auto rsc = __builtin_amdgcn_make_buffer_rsrc(p.C + obase, (short)0, TM * N * 2, 0x00020000);
  const int qv = ((lane & 15) * N + w.wn * TN + swap16_col(lane)) * 2;
  typedef unsigned u32x4 __attribute__((ext_vector_type(4)));"""
_BST_OLD2 = """      st16(p.Y + rowoff + npc + pp * 32, yp[pp]);
      st16(p.C + rowoff + npc + pp * 32, cpk[pp]);"""
_BST_NEW2 = """      if constexpr (MODE == NT_FWD) {
        __builtin_amdgcn_raw_buffer_store_b128(u32x4{yp[pp].x, yp[pp].y, yp[pp].z, yp[pp].w}, rsy, qv + pp * 64,
                                               j * 16 * N * 2, 0);
        __builtin_amdgcn_raw_buffer_store_b128(u32x4{cpk[pp].x, cpk[pp].y, cpk[pp].z, cpk[pp].w}, rsc,
                                               qv + pp * 64, j * 16 * N * 2, 0);
      } else {
        st16(p.Y + rowoff + npc + pp * 32, yp[pp]);
        st16(p.C + rowoff + npc + pp * 32, cpk[pp]);
      }"""

# fused head (NT_FWD_HB) cost split: no hand-off (each block uses its own partial for all column
# tiles: WRONG g, timing only)
_HB_WAIT_OLD = """        while ((u = __hip_atomic_load(hpu + (size_t)jt * p.M + m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) ==
               kHeadPending) {"""
_HB_WAIT_NEW = """        u = __float_as_uint(own) + jt;
        while (polls == 12345) {"""

# forward stores folded onto the first 512 rows of Y / C (1 MB each: L2-resident, no HBM write-back):
# WRONG outputs, timing only -- prices the forward's 4.3 GB of output writes against HBM
_L2ST_OLD = """      st16(p.Y + rowoff + npc + pp * 32, yp[pp]);
      st16(p.C + rowoff + npc + pp * 32, cpk[pp]);"""
_L2ST_NEW = """      st16(p.Y + (rowoff & (size_t)(512 * p.N - 1)) + npc + pp * 32, yp[pp]);
      st16(p.C + (rowoff & (size_t)(512 * p.N - 1)) + npc + pp * 32, cpk[pp]);"""

# forward epilogue computes everything but issues no stores (a never-true guard keeps the values):
# WRONG outputs, timing only -- the epilogue's VALU alone against its stores
_NOST_NEW = """      if (yp[pp].x == 0x12345u && cpk[pp].y == 0x6789u) {
        st16(p.Y + rowoff + npc + pp * 32, yp[pp]);
        st16(p.C + rowoff + npc + pp * 32, cpk[pp]);
      }"""

# dW GEMM operands from 8 K-steps of the slice only (L2-resident Y and dZ): WRONG dW, timing only --
# prices the dW K-loop's operand latency
_DWL2_OLD = """        const int ks = ks_begin + min(kt, nkl - 1);  // past the slice: a consumed piece re-read"""
_DWL2_NEW = """        const int ks = ks_begin + (min(kt, nkl - 1) & 7);"""

# ping-pong K-loops without the s_setprio around each MFMA cluster (the barriers alone order the
# two wave groups; bit-identical) -- timing only
_PRIO_OLD1 = """      __builtin_amdgcn_s_setprio(1);
      mma(ph);       // each MFMA waits (counted lgkmcnt) only for its fragments
      wait_lgkm0();  // every read of this slot has landed before the barrier that frees it
      __builtin_amdgcn_s_setprio(0);"""
_PRIO_NEW1 = """      mma(ph);
      wait_lgkm0();"""
_PRIO_OLD2 = """      __builtin_amdgcn_s_setprio(1);
      mma(sg);
      __builtin_amdgcn_s_setprio(0);"""
_PRIO_NEW2 = """      mma(sg);"""

VARIANTS = {
    "noprio": {"gemm_pipeline.h": [(_PRIO_OLD1, _PRIO_NEW1), (_PRIO_OLD2, _PRIO_NEW2)]},
    "dw_l2": {"gemm_tn.hip": [(_DWL2_OLD, _DWL2_NEW)]},
    "st_none": {"gemm_nt.hip": [(_L2ST_OLD, _NOST_NEW)]},
    "st_l2": {"gemm_nt.hip": [(_L2ST_OLD, _L2ST_NEW)]},
    "hb_nowait": {"gemm_nt.hip": [(_HB_WAIT_OLD, _HB_WAIT_NEW)]},
    "bst": {"gemm_nt.hip": [(_BST_OLD1, _BST_NEW1), (_BST_OLD2, _BST_NEW2)]},
    "st_sc1": {"gemm_nt.hip": [(_ST16, _st16_asm("sc1"))]},          # write-through epilogue stores
    "st_nt": {"gemm_nt.hip": [(_ST16, _st16_asm("nt"))]},            # non-temporal epilogue stores
    "st_sc0sc1": {"gemm_nt.hip": [(_ST16, _st16_asm("sc0 sc1"))]},
}


# the Snake / Tanh forward with 16-row store pieces at every K (the product takes whole lines at K <= 512)
VARIANTS["actplain"] = {"gemm_nt.hip": [("(Cfg::PP && p.K <= 512)", "(Cfg::PP && p.K <= 0)")]}

# the first layer's Y0 / C0 stores non-temporal
VARIANTS["ffnt"] = {"elementwise.hip": [
    ("    *(h16x8*)(Y0 + m * ld + n) = yv;\n    if constexpr (STORE_C) *(h16x8*)(C0 + m * ld + n) = cv;",
     "    __builtin_nontemporal_store(yv, (h16x8*)(Y0 + m * ld + n));\n"
     "    if constexpr (STORE_C) __builtin_nontemporal_store(cv, (h16x8*)(C0 + m * ld + n));")]}


# LDS-DMA issue one statement per DMA (siren_common.h SIREN_GLDS_PAIR 0: the round-5 issue path; the
# product issues a staging piece's two DMAs under one M0 value)
VARIANTS["glds0"] = {}
# plain (write-back) whole-line epilogue stores instead of non-temporal ones (gemm_nt.hip SIREN_NT_STNT)
VARIANTS["stnt0"] = {}
# the whole-line epilogue stores with `sc1` (inline asm, saddr form): gfx950 drops an sc1-stored line from
# the XCD's L2 instead of keeping it (MI355X_MICROARCH.md store table) -- do 8 MB of Y / C per tile round
# stop evicting W and X?  (asm stores are invisible to hipcc's vmcnt counting: its waits only get stricter;
# the s_nop covers the store-data VGPR write hazard hipcc cannot see inside asm, as _st16_asm's)
_STSC1 = ('    stl((h16*)(ub + (size_t)(16 * q) * w.LD + lq), line[q]);',
          '    { typedef unsigned u32x4 __attribute__((ext_vector_type(4)));\n'
          '      asm volatile("global_store_dwordx4 %0, %1, %2 sc1\\n\\ts_nop 1" :: "v"(lq), "v"(__builtin_bit_cast(u32x4, line[q])),\n'
          '                   "s"(ub + (size_t)(16 * q) * w.LD) : "memory"); }')
VARIANTS["stsc1"] = {"gemm_nt.hip": [_STSC1]}
# PROBE (wrong outputs, timing only): group 0 (waves 0-3) issues every LDS-DMA and stores nothing, group 1
# (waves 4-7) stores its own lines twice (its rows and group 0's: the same bytes) and never waits on vmcnt
# in the K-loop -- the forward's K-loop waits then no longer sit behind the epilogue's stores in any
# wave's in-order vmcnt.  Prices that coupling (10.8 k cycles per tile) before an LDS
# hand-off of group 0's outputs is built.  Non-EARLY K-loop only (the plain forward).
VARIANTS["dmag0"] = {"gemm_nt.hip": [
    ("""    int urow[4][2];
    unsigned pdst[4][2];""",
     """    int urow[4][2], urowp[4][2];
    unsigned pdst[4][2], pdstp[4][2];"""),
    ("""        urow[pc][j] = lr0 * K * 2;
        pdst[pc][j] = ((pc & 1) ? 0u : (unsigned)Cfg::XBYTES) + (unsigned)(lr0 * ROWB);
      }""",
     """        urow[pc][j] = lr0 * K * 2;
        pdst[pc][j] = ((pc & 1) ? 0u : (unsigned)Cfg::XBYTES) + (unsigned)(lr0 * ROWB);
        const int qr0 = (2 * (wave + 4) + j) * 8;
        const int lq0 = (pc & 1) ? (qr0 >> 6) * 128 + (qr0 & 63) + 64 * hf : (qr0 >> 5) * 64 + (qr0 & 31) + 32 * hf;
        urowp[pc][j] = lq0 * K * 2;
        pdstp[pc][j] = ((pc & 1) ? 0u : (unsigned)Cfg::XBYTES) + (unsigned)(lq0 * ROWB);
      }"""),
    ("""        glds16x2o_asm_s(lane_src, lane_src8, (const char*)src + urow[PC][0], lds_addr(dst + pdst[PC][0]));
      } else {""",
     """        if (wm == 0) {
          glds16x2o_asm_s(lane_src, lane_src8, (const char*)src + urow[PC][0], lds_addr(dst + pdst[PC][0]));
          glds16x2o_asm_s(lane_src, lane_src8, (const char*)src + urowp[PC][0], lds_addr(dst + pdstp[PC][0]));
        }
      } else {"""),
    ("""    stl((h16*)(ub + (size_t)(16 * q) * w.LD + lq), line[q]);
  }
}""",
     """    if (w.wm == 1) {
      stl((h16*)(ub + (size_t)(16 * q) * w.LD + lq), line[q]);
      stl((h16*)(ub - (size_t)256 * w.LD + (size_t)(16 * q) * w.LD + lq), line[q]);
    }
  }
}"""),
  ],
  "gemm_pipeline.h": [
    ("""    if constexpr (EARLY) {
    issue(0, 1, 1, phase_t<3>{});
    wait_vmcnt<10>();  // K-tile 0's pieces 0..2 have landed (K0 p3, K1 p0..3 younger)
  } else {
    wait_vmcnt<8>();  // K-tile 0's pieces 0..2 (and the older ones) have landed
  }""".replace("    if constexpr (EARLY) {", "  if constexpr (EARLY) {"),
     """  if constexpr (EARLY) {
    issue(0, 1, 1, phase_t<3>{});
    wait_vmcnt<10>();  // K-tile 0's pieces 0..2 have landed (K0 p3, K1 p0..3 younger)
  } else {
    if (grp == 0) wait_vmcnt<16>();
  }"""),
    ("""      constexpr bool R = RELAXED || (SG == 0 && RELAXED_A);
      wait_vmcnt<R ? 8 + E : 8>();""",
     """      if (grp == 0) wait_vmcnt<16>();"""),
  ]}
# its store half alone (both groups issue their DMAs and wait as in the product): group 1 stores its lines
# twice, group 0 none (wrong outputs, timing only) -- dmag0 minus this = the DMA / store decoupling
VARIANTS["st1x2"] = {"gemm_nt.hip": [VARIANTS["dmag0"]["gemm_nt.hip"][3]]}
# every ping-pong NT kernel with the EARLY tile boundary (the product takes it for the fused last layer and
# dX0 only): round 5 measured the plain forward +2.3% at cfg2 and -2.3% at cfg4 -- a K-dependent choice?
VARIANTS["early"] = {}
DEFINES = {"glds0": ("SIREN_GLDS_PAIR=0",), "stnt0": ("SIREN_NT_STNT=0",), "early": ("SIREN_NT_EARLY=1",)}


def apply(name: str) -> dict:
    """{file: patched text} of variant `name` against the sources in csrc (text only, nothing
    compiled); raises ValueError for a patch whose target is no longer there."""
    patched = {}
    for f, reps in VARIANTS[name].items():
        s = open(os.path.join(CSRC, f)).read()
        for old, new in reps:
            if old not in s:
                raise ValueError(f"variant {name}: patch target not found in {f}: {old.strip()[:60]!r}")
            s = s.replace(old, new)
        patched[f] = s
    return patched


def check() -> list:
    """What a kernel edit broke: every variant's patches must apply, and every macro named in
    DEFINES must still be a compile-time knob (#ifndef) of some source."""
    problems = []
    for name in VARIANTS:
        try:
            apply(name)
        except ValueError as e:
            problems.append(str(e))
    text = "".join(open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)))
    for name, defines in DEFINES.items():
        if name not in VARIANTS:
            problems.append(f"DEFINES names an unknown variant {name}")
        for d in defines:
            macro = d.split("=")[0]
            if not re.search(rf"^#ifndef {macro}\b", text, flags=re.M):
                problems.append(f"variant {name}: no #ifndef {macro} under csrc")
    return problems


def build(name: str, extra_defines=()) -> str:
    extra_defines = (*DEFINES.get(name, ()), *extra_defines)
    try:
        patched = apply(name)
    except ValueError as e:
        raise SystemExit(str(e))
    out = os.path.join(ROOT, "inr-for-audio_amd", f"libsiren_{name}.so")
    with tempfile.TemporaryDirectory() as tmp:
        for f in os.listdir(CSRC):
            shutil.copy(os.path.join(CSRC, f), tmp)
        for f, s in patched.items():
            open(os.path.join(tmp, f), "w").write(s)
        capi = os.path.join(tmp, "capi.hip")
        s = open(capi).read().replace('"../../include/siren_hip.h"', f'"{ROOT}/include/siren_hip.h"')
        open(capi, "w").write(s)
        cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17",
               "-fPIC", "-shared", "-ffp-contract=off", *[f"-D{d}" for d in extra_defines],
               *[os.path.join(tmp, f) for f in SOURCES], "-o", out]
        subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)
    return out


if __name__ == "__main__":
    if sys.argv[1:] == ["--check"]:
        bad = check()
        print("\n".join(bad) if bad else f"{len(VARIANTS)} variants apply")
        sys.exit(1 if bad else 0)
    for nm in sys.argv[1:]:
        print(build(nm))
