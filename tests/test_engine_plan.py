"""What an engine decides before it allocates (csrc/engine_plan.hpp:
resolve_schedule, plan_engine), checked without a GPU: a stand-alone host
program (tests/engine_plan/plan_check.cpp: engine_plan.hpp and graph.cpp's
loader only, its own main, no HIP) compiled with g++ under AddressSanitizer +
UBSan into pytest's tmp_path and run directly.  It prints one line per case;
the expectations below were derived by hand from the rules as Engine::init
stated them before they became a function: the DNA code (N = 18432, M = 2048,
E = 147456, 2 509 064 bytes per codeword) with 200 GB free, and synthetic
graphs on either side of each rule.

var_cpw: 3 is kept (include/ldpc_amd.h: "3: compressed min-sum only"), as
every engine before this function did; 0, 5, 6, 7 and 9 become -2."""
import os
import subprocess

from conftest import PCHK, ROOT


def _plan(res=0, cont=1, msa_c=0, handover=0, nt=None, first_fp=0, syn=None, cap=0, group=None, c2v_tiles=None,
          c2v_bytes=0, no_drain=0, bad_lane=0):
    tiles = cap // 64
    nt = (0 if res else 1) if nt is None else nt
    syn = (32 if cont and not res else 0) if syn is None else syn
    group = tiles if group is None else group
    c2v_tiles = tiles if c2v_tiles is None else c2v_tiles
    return (f"msa_c={msa_c} cont={cont} res={res} handover={handover} nt={nt} first_fp={first_fp} no_drain={no_drain} "
            f"bad_lane={bad_lane} cpw=-2 poll=8 syn={syn} cap={cap} cap_tiles={tiles} group={group} "
            f"c2v_tiles={c2v_tiles} c2v_bytes={c2v_bytes}")


E_DNA = 147456
G3 = 3 * 64 * E_DNA * 8  # fp64 scratch of a 3-tile group
FIXED = _plan(cont=0, cap=16384, group=3, c2v_tiles=3, c2v_bytes=G3)

EXPECTED = {
    "dna": "M=2048 N=18432 E=147456 dc=72 dv=8 bytes_per_codeword=2509064",
    # resident pool of 3 tiles, hand-over, cached (no nontemporal), syndrome in the check kernel
    "bp": _plan(res=1, handover=1, cap=192),
    # compressed, continuous, 1024 lanes in groups of 8; scratch: 8 tiles x M x 64 x (4 fp64 + 1 u16)
    "msa": _plan(msa_c=1, cap=1024, group=8, c2v_tiles=8, c2v_bytes=8 * 2048 * 64 * 34),
    # an explicit pool above 4 tiles: grouped, first check from the prior, scratch max(3, (5 + 3) / 4) tiles
    "bp chunk=320": _plan(first_fp=1, cap=320, group=3, c2v_tiles=max(3, (5 + 3) // 4), c2v_bytes=G3),
    "bp chunk=320 resident": _plan(res=1, handover=1, cap=320),
    "bp fixed": FIXED,
    "qmsa": FIXED,
    "gallager_a": FIXED,
    "gallager_b1": FIXED,
    "gallager_b2": FIXED,
    "bp no handover": _plan(res=1, handover=0, cap=192),
    "bp chunk=4194304": "error=chunk too large (max 4194240 codewords)",
    "bp chunk=4194240": _plan(first_fp=1, cap=4194240, group=3, c2v_tiles=(65535 + 3) // 4,
                              c2v_bytes=16384 * 64 * E_DNA * 8),
    # 10 MB free: 5 MB / 2 509 064 = 1 codeword, rounded up to one tile
    "bp little memory": _plan(res=1, handover=1, cap=64),
    "msa little memory": _plan(msa_c=1, cap=64, c2v_bytes=2048 * 64 * 34),
    "bp debug": _plan(res=1, handover=1, cap=192, no_drain=1, bad_lane=1),
    # (8, 72)-regular, N = 36864: 3 tiles would take 509 MB > 1.15 x 226 MB, so grouped by default;
    # E = 294912 >= 2^18: no compressed min-sum
    "big": "M=4096 N=36864 E=294912 dc=72 dv=8 regular=11",
    "big bp": _plan(first_fp=1, cap=16384, group=3, c2v_tiles=64, c2v_bytes=64 * 64 * 294912 * 8),
    "big bp resident": _plan(res=1, handover=1, cap=192),
    "big msa": _plan(cap=16384, group=3, c2v_tiles=64, c2v_bytes=64 * 64 * 294912 * 8),
    # a column of degree 33: no register bucket, fixed passes (E = 113)
    "dv33": "dc=3 dv=33",
    "dv33 bp": _plan(cont=0, cap=16384, group=3, c2v_tiles=3, c2v_bytes=3 * 64 * 113 * 8),
    # a row of degree 97: continuous, but no register bucket for the in-place check (E = 254)
    "dc97": "dc=97 dv=4",
    "dc97 bp": _plan(cap=16384, group=3, c2v_tiles=64, c2v_bytes=64 * 64 * 254 * 8),
    "dc97 msa": _plan(cap=16384, group=3, c2v_tiles=64, c2v_bytes=64 * 64 * 254 * 8),
    # (4, 32)-regular: the generic resident pool, floor(226e6 / (512 x (8192 + 2048))) = 43 tiles
    "reg4x32": "M=256 N=2048 E=8192 dc=32 dv=4 regular=11 pool_tiles=43",
    "reg4x32 bp": _plan(res=1, cap=64 * 43),
    "reg4x32 msa": _plan(res=1, cap=64 * 43),
    "reg4x32 bp pool_tiles=2": _plan(res=1, cap=128),
    # Regular on one side only (a specialised kernel next to a generic one).  None is (8, 72)-regular, so
    # no compressed min-sum, hand-over or first check from the prior, and the resident pool comes from
    # gen_res alone (both degrees in a register bucket), which puts no condition on N.
    # (6, 72)-regular, N = 360 (N % 32 = 8): rows in check bucket 96, columns in variable bucket 8 -> resident;
    # E = 30 x 72 = 2160, pool of floor(226e6 / (512 x (2160 + 360))) = floor(226e6 / 1290240) = 175 tiles
    "reg6x72": "M=30 N=360 E=2160 dc=72 dv=6 regular=11 pool_tiles=175",
    "reg6x72 bp": _plan(res=1, cap=64 * 175),
    "reg6x72 msa": _plan(res=1, cap=64 * 175),
    "reg6x72 bp resident": _plan(res=1, cap=64 * 175),
    "reg6x72 msa resident": _plan(res=1, cap=64 * 175),
    # an explicit pool of 5 tiles > kResAutoMaxTiles = 4: grouped unless the caller chose RESIDENT;
    # scratch max(3, (5 + 3) / 4) = 3 tiles of 64 x 2160 fp64
    "reg6x72 bp chunk=320": _plan(cap=320, group=3, c2v_tiles=3, c2v_bytes=3 * 64 * 2160 * 8),
    "reg6x72 bp chunk=320 resident": _plan(res=1, cap=320),
    # (8, 48)-regular, N = 240: continuous by its columns (degree 8), check bucket 48 -> resident;
    # E = 40 x 48 = 1920, floor(226e6 / (512 x (1920 + 240))) = floor(226e6 / 1105920) = 204 tiles
    "reg8x48": "M=40 N=240 E=1920 dc=48 dv=8 regular=11 pool_tiles=204",
    "reg8x48 bp": _plan(res=1, cap=64 * 204),
    "reg8x48 msa": _plan(res=1, cap=64 * 204),
    "reg8x48 bp resident": _plan(res=1, cap=64 * 204),
    "reg8x48 msa resident": _plan(res=1, cap=64 * 204),
    # (8, 100)-regular, N = 300: rows past the last check bucket (96), so never resident, whatever the
    # caller sets: the grouped schedule over 16384 lanes = 256 tiles, groups of 3, scratch
    # max(3, (256 + 3) / 4) = 64 tiles of 64 x E fp64, E = 24 x 100 = 2400;
    # gen_pool_tiles (not used): floor(226e6 / (512 x (2400 + 300))) = floor(226e6 / 1382400) = 163
    "reg8x100": "M=24 N=300 E=2400 dc=100 dv=8 regular=11 pool_tiles=163",
    "reg8x100 bp": _plan(cap=16384, group=3, c2v_tiles=64, c2v_bytes=64 * 64 * 2400 * 8),
    "reg8x100 msa": _plan(cap=16384, group=3, c2v_tiles=64, c2v_bytes=64 * 64 * 2400 * 8),
    "reg8x100 bp resident": _plan(cap=16384, group=3, c2v_tiles=64, c2v_bytes=64 * 64 * 2400 * 8),
    "reg8x100 msa resident": _plan(cap=16384, group=3, c2v_tiles=64, c2v_bytes=64 * 64 * 2400 * 8),
    # resolve_schedule.  All known bits 0xf0b9, the defaults 0x30b9 (the two debug bits off); bit 30 marks
    # a resolved schedule, bit 29 a caller that chose RESIDENT itself
    "null": "set=0x4000f0b9 flags=0x30b9 group=-2 cpw=-2 pool=0 poll=8 syn=32 reserved=0",
    # every bit set by the caller but RESIDENT's value: unknown bits dropped
    "unknown bits": "set=0x6000f0b9 flags=0xf099 group=-2 cpw=-2 pool=0 poll=8 syn=32 reserved=0",
    # bits 30 and 29 set by a caller: dropped, and every field resolved as a caller's
    "marked resolved": "set=0x4000f0b9 flags=0x30b9 group=-2 cpw=-2 pool=0 poll=8 syn=256 reserved=0",
    "var_cpw 0 -> -2": None, "var_cpw 1 -> 1": None, "var_cpw 2 -> 2": None, "var_cpw 3 -> 3": None,
    "var_cpw 4 -> 4": None, "var_cpw 5 -> -2": None, "var_cpw 6 -> -2": None, "var_cpw 7 -> -2": None,
    "var_cpw 8 -> 8": None, "var_cpw 9 -> -2": None,
    "kept": "set=0x4000f0b9 flags=0x30b9 group=-1 cpw=-2 pool=5 poll=3 syn=256 reserved=0",
}


def test_engine_plan_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-static-libasan", "-static-libubsan",  # the runtimes inside the program itself
                           "-o", exe, os.path.join(ROOT, "tests", "engine_plan", "plan_check.cpp"),
                           os.path.join(ROOT, "dna-ldpc-codes_amd", "csrc", "graph.cpp")])
    r = subprocess.run([exe, PCHK], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    want = [k if v is None else f"{k}: {v}" for k, v in EXPECTED.items()]
    got = r.stdout.splitlines()
    for g, w in zip(got, want):
        assert g == w
    assert len(got) == len(want), got[len(want):] or want[len(got):]
