"""CPU-side checks of the product: the C-ABI library loads and exports every symbol
include/gr4pm_hip.h declares, the one-wave FFT index algebra is right (host emulation of the
64 lanes), host-only helpers match the oracle, and the product refuses to run without a GPU
(no CPU fallback).  No compute calls need a GPU here."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import __graft_entry__ as ge
import _oracle as orc

ROOT = ge.ROOT


@pytest.fixture(scope="module")
def pkg():
    if not os.path.exists(os.path.join(ge.PKG_DIR, "libgr4pm_hip.so")):
        ge.build()
    return ge.load_package()


def test_library_exports_every_declared_symbol(pkg):
    header = open(os.path.join(ROOT, "include", "gr4pm_hip.h")).read()
    declared = sorted(set(re.findall(r"\b(gr4pm_[a-z0-9_]+)\s*\(", header)))
    assert declared, "no declarations parsed"
    L = pkg.lib()
    missing = [s for s in declared if not hasattr(L, s)]
    assert not missing, missing
    assert sorted(pkg.EXPORTS) == declared
    assert b"gfx950" in L.gr4pm_version()


def test_no_cpu_fallback_without_gpu(pkg):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    rrc, _ = orc.unit_norm_rrc(4)
    with pytest.raises(pkg.Gr4pmError):
        pkg.SyncwordDetection(rrc, np.zeros(64, np.uint8), np.array([1, -1], np.complex64))
    with pytest.raises(pkg.Gr4pmError):
        pkg.Rotator(0.1)


def test_every_abi_entry_point_has_an_exception_guard():
    """include/gr4pm_hip.h: "No exceptions cross the ABI".  tools/check_abi_guards.py reads csrc/*.hip and fails when
    an extern "C" definition is neither a function-try-block ending in GR4PM_ABI_CATCH* nor on its no-throw list."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_abi_guards.py")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_bad_alloc_inside_an_entry_point_comes_back_as_a_status(pkg):
    """test-only allocator hook (gr4pm_test_fail_allocations, TEST build of the library only: tests/gr4pm_test_hooks.h):
    the std::vector inside the RRC design throws std::bad_alloc; the entry point returns 0 taps and the error text
    instead of unwinding into the caller.  The hook only sees the library's own allocations and disarms itself after
    the failure.  The shipped library has neither the entry points nor an operator new of its own."""
    shipped = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "gr4pm_test_" not in shipped and "_Znwm" not in shipped and not hasattr(pkg.lib(), "gr4pm_test_fail_allocations")
    all_syms = subprocess.run(["nm", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert " _Znwm" not in all_syms, "the shipped library must not replace operator new"
    pkg = ge.load_test_build()
    L = pkg.lib()
    before = L.gr4pm_test_allocation_count()
    assert pkg.root_raised_cosine(1.0, 4.0, 1.0, 0.35, 65).size == 65
    assert L.gr4pm_test_allocation_count() > before  # the library's operator new is the one in use
    L.gr4pm_test_fail_allocations(0, 1)
    assert pkg.root_raised_cosine(1.0, 4.0, 1.0, 0.35, 65).size == 0
    assert b"bad_alloc" in L.gr4pm_last_error()
    assert pkg.root_raised_cosine(1.0, 4.0, 1.0, 0.35, 65).size == 65  # disarmed again
    np.zeros(1 << 20)  # allocations of the rest of the process never saw the hook
    L.gr4pm_test_fail_allocations(-1, 0)


def test_occupancy_guard_trips_on_a_widened_kernel(pkg, tmp_path):
    """tools/check_occupancy.py (run by build()): the budgets the pipelined receiver's co-residency rests on -- the
    correlator at <= 240 VGPRs, exactly 151 552 bytes of LDS and no scratch; the two serial kernels at <= 32 VGPRs --
    are read back from the code objects in the built library.  The built library passes; one more __shared__ word in
    the correlator, a 34-register PLL, a spilling correlator or a renamed kernel is reported.  And the reader itself,
    on a freshly compiled kernel with known LDS and a forced register count."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_occupancy as oc
    rows = oc.table(pkg.LIB_PATH)
    assert len(rows) > 60 and oc.check(rows) == []
    by = {r["kernel"]: r for r in rows}
    corr = next(k for k in by if "k_correlate_w64ILi114688E" in k)
    pll = next(k for k in by if "k_costas_capILi1ELi2E" in k)
    rot = next(k for k in by if "k_rot_checkpoints" in k)
    assert by[corr]["vgpr"] <= 240 and by[corr]["lds_bytes"] == 151552 and by[corr]["scratch_bytes"] == 0
    assert by[pll]["vgpr"] <= 32 and by[rot]["vgpr"] <= 32

    def widened(name, **change):
        return [dict(r, **change) if r["kernel"] == name else r for r in rows]

    assert any("LDS" in e for e in oc.check(widened(corr, lds_bytes=151552 + 4)))
    assert any("VGPRs" in e for e in oc.check(widened(corr, vgpr=248)))
    assert any("scratch" in e for e in oc.check(widened(corr, scratch_bytes=16)))
    assert any("VGPRs" in e and "k_costas_cap" in e for e in oc.check(widened(pll, vgpr=34)))
    assert any("VGPRs" in e and "k_rot_checkpoints" in e for e in oc.check(widened(rot, vgpr=40)))
    # (round 6: three kernels carry the name -- the generic one, _fresh, _both; the guard speaks up when none is left)
    assert any("no kernel matches" in e for e in oc.check([r for r in rows if "k_rot_checkpoints" not in r["kernel"]]))
    assert sum("k_rot_checkpoints" in k for k in by) == 3 and all(by[k]["vgpr"] <= 32 and by[k]["scratch_bytes"] == 0
                                                                 for k in by if "k_rot_checkpoints" in k)
    src = tmp_path / "wide.hip"
    src.write_text("""#include <hip/hip_runtime.h>
__global__ __launch_bounds__(64) void k_rot_checkpoints(float* p) {
    __shared__ float pad[3 * 1024 + 1];   // 12 292 bytes: four more than what is free beside the correlator
    float v[48];
    for (int i = 0; i < 48; ++i) v[i] = p[threadIdx.x + 64 * i];
    pad[threadIdx.x] = v[0]; __syncthreads();
    float s = pad[63 - threadIdx.x];
    for (int i = 0; i < 48; ++i) s = s * v[i] + v[47 - i];
    p[threadIdx.x] = s;
}
""")
    so = tmp_path / "wide.so"
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "--offload-arch=gfx950", "-shared", "-fPIC", "-o", str(so), str(src)])
    wide = oc.table(str(so))
    assert len(wide) == 1 and wide[0]["lds_bytes"] == 12292 and wide[0]["vgpr"] > 32
    errors = [e for e in oc.check(wide) if "k_rot_checkpoints" in e and "no kernel" not in e]
    assert any("VGPRs" in e for e in errors) and any("LDS" in e for e in errors), errors


def test_isa_guard_catches_what_it_is_there_for(tmp_path):
    """tools/check_m0.py on hand-made assembly: a register of an asm-issued template load touched before the
    s_waitcnt that covers it, a compiler-generated m0 write (also in the v_readfirstlane form) and scratch use are
    each reported; the same code with the wait in place passes"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_m0
    head = ("_Z15k_correlate_w64ILi1EEvv:\n; %bb.0:\n\ts_mov_b32 s4, 0\n.LBB0_1:   ; in Loop: Header=BB0_1 Depth=1\n"
            "\t;;#ASMSTART\n\tglobal_load_dwordx4 v[0:3], v9, s[2:3] offset:1024\n\t;;#ASMEND\n"
            "\tglobal_store_dword v8, v7, s[4:5]\n")
    tail = ("\tv_add_f32_e32 v5, v1, v6\n\ts_cbranch_scc1 .LBB0_1\n; %bb.2:\n\ts_endpgm\n.Lfunc_end0:\n"
            "\t.amdhsa_kernel _Z15k_correlate_w64ILi1EEvv\n\t\t.amdhsa_private_segment_fixed_size {scr}\n\t.end_amdhsa_kernel\n")

    def run(body, scr=0):
        f = tmp_path / "k.s"
        f.write_text(head + body + tail.format(scr=scr))
        return check_m0.check(str(f))[-1]

    assert run("\t;;#ASMSTART\n\ts_waitcnt vmcnt(1)\n\t;;#ASMEND\n") == []            # the store may stay in flight
    bad = run("\t;;#ASMSTART\n\ts_waitcnt vmcnt(2)\n\t;;#ASMEND\n")                    # ... the load may not
    assert len(bad) == 1 and "v1 is still being loaded" in bad[0]
    assert any("still being loaded" in b for b in run(""))                                # no wait at all (loop path too)
    assert any("write of m0" in b for b in run("\ts_waitcnt vmcnt(0)\n\tv_readfirstlane_b32 m0, v4\n"))
    assert any("scratch" in b for b in run("\ts_waitcnt vmcnt(0)\n", scr=16))


def test_library_exports_only_the_c_abi(pkg):
    """csrc/exports.map: nothing but gr4pm_* is in the dynamic symbol table -- in particular not the library's own
    operator new / delete, which would otherwise interpose on every C++ allocation of the process"""
    r = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True, check=True)
    names = [l.split()[-1] for l in r.stdout.splitlines() if l.strip()]
    assert names and all(n.startswith("gr4pm_") for n in names), [n for n in names if not n.startswith("gr4pm_")][:5]


def test_firdes_matches_oracle_and_reference_vector(pkg):
    for args in [(1.0, 4.0, 1.0, 0.35, 44), (32.0, 128.0, 1.0, 0.35, 1408), (1.0, 4.0, 1.0, 0.35, 65)]:
        got = pkg.root_raised_cosine(*args)
        want = orc.rrc_taps(*args)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    expected = np.load(os.path.join(ROOT, "tests", "golden", "qa_firdes_rrc65.npy"))
    assert np.all(np.abs(pkg.root_raised_cosine(1.0, 4.0, 1.0, 0.35, 65) - expected) < 1e-7)


def test_default_pfb_arb_taps_blob(pkg):
    taps = pkg.default_pfb_arb_taps()
    assert taps.size == 1280  # pfb_arb_taps.hpp:8-12: 32 arms x 40 taps
    assert np.array_equal(taps, np.load(os.path.join(ROOT, "tests", "golden", "ref_pfb_arb_taps.npy")))


def test_one_wave_fft_schedules_host_emulation(tmp_path):
    """runs the 64 lanes of fft2048_wave.hpp phase by phase on the CPU against a double DFT"""
    exe = tmp_path / "fft_wave_emu"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ge.PKG_DIR, "csrc"), "-o", str(exe),
                           os.path.join(ROOT, "tests", "fft_wave_emu.cpp")])
    out = subprocess.check_output([str(exe)]).decode()
    m = re.findall(r"fft(\d) relerr ([0-9.e+-]+) coverage_bad (\d+)", out)
    assert len(m) == 4  # FFT-1, FFT-2 by one wave; the same by a pair of waves (fft2048_pair.hpp)
    for _, err, bad in m:
        assert float(err) < 5e-7 and int(bad) == 0
    # the pair schedules do the same arithmetic in another distribution: identical bits
    assert re.search(r"pair_vs_wave_differing_values 0\b", out)


def test_one_exchange_wave_fft_host_emulation(tmp_path):
    """fft2048_w64.hpp (the correlator's 32 x 64 schedule, one LDS exchange per transform): the 64 lanes run
    phase by phase on the CPU, both exchange layouts, against a double DFT"""
    exe = tmp_path / "fft_w64_emu"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ge.PKG_DIR, "csrc"), "-o", str(exe),
                           os.path.join(ROOT, "tests", "fft_w64_emu.cpp")])
    out = subprocess.check_output([str(exe)]).decode()
    errs = [float(e) for e in re.findall(r"max_rel_err ([0-9.e+-]+)", out)]
    assert len(errs) == 6 and max(errs) < 5e-7, out   # incl. the planar pass B of the per-bin transforms


def test_glibc_sinf_cosf_restatement_matches_the_host_libm(tmp_path):
    """tests/sincosf_glibc_check.c: the double-precision sinf / cosf algorithm the Costas kernels use
    (csrc/costas_loop.hip: sincosf_glibc) against the host libm the reference calls, for EVERY float of
    |x| <= 3.2 (the loop phase lives in [-pi, pi)), with and without FMA contraction"""
    for fma in (1, 0):
        exe = tmp_path / f"sc{fma}"
        subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", f"-DFMA={fma}"] + (["-march=native"] if fma else []) +
                              ["-o", str(exe), os.path.join(ROOT, "tests", "sincosf_glibc_check.c"), "-lm", "-lpthread"])
        out = subprocess.check_output([str(exe)]).decode()
        assert re.search(r"sin mismatches 0, cos mismatches 0", out), out


def test_fft4096_workgroup_schedule_host_emulation(tmp_path):
    """fft4096_wg.hpp (configs[4]: 16 x 16 x 16, 256 threads): the threads run phase by phase on the CPU"""
    exe = tmp_path / "fft4096_emu"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ge.PKG_DIR, "csrc"), "-o", str(exe),
                           os.path.join(ROOT, "tests", "fft4096_emu.cpp")])
    out = subprocess.check_output([str(exe)]).decode()
    errs = [float(e) for e in re.findall(r"max_rel_err ([0-9.e+-]+)", out)]
    assert len(errs) == 2 and max(errs) < 5e-7, out


def test_packet_transmitter_rrc_taps_computed_in_product(pkg):
    """packet_transmitter_rrc_taps.hpp:8-28 restated over the library's own firdes: bit-exact against the taps
    the reference's header produced (tests/golden/ref_txrrc_4.npy, built by oracle/_ref)"""
    got = pkg.packet_transmitter_rrc_taps(4)
    ref = np.load(os.path.join(ROOT, "tests", "golden", "ref_txrrc_4.npy"))
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))


def test_bench_roofline_traffic_comes_from_the_committed_counters(monkeypatch):
    """roofline.traffic is read from profiles/ at run time (never a constant in bench.py) and only for the kernel the
    counters were taken on: another correlator kernel gets null and a reason"""
    import bench
    samples = 67106856
    t = bench.pmc_traffic(samples, "k_correlate_w64")
    assert t["traffic"] is not None and 11.5 * samples < t["traffic"] < 13.5 * samples
    assert "_k_correlate_hbm_traffic.json" in t["traffic_source"]
    other = bench.pmc_traffic(samples, "k_correlate")
    assert other["traffic"] is None and "describes" in other["traffic_source"]
    assert t["traffic_measured"] is False and other["traffic_measured"] is False
    monkeypatch.setenv("GR4PM_CORRELATOR", "wave")
    assert bench.correlator_kernel() == "k_correlate"
    monkeypatch.delenv("GR4PM_CORRELATOR")
    assert bench.correlator_kernel() == "k_correlate_w64"
    # round 6: what measure_traffic_in_run() measured in the run wins over the committed file -- for its own kernel only
    monkeypatch.setattr(bench, "MEASURED_TRAFFIC", {"bytes_per_launch": 12.1 * samples, "bytes_per_sample": 12.1, "samples": samples,
                                                    "read_bytes_corrected": 8.1 * samples, "write_bytes": 4.0 * samples,
                                                    "kernel": "k_correlate_w64"})
    m = bench.pmc_traffic(2 * samples, "k_correlate_w64")
    assert m["traffic_measured"] is True and m["traffic"] == round(12.1 * 2 * samples) and "this run" in m["traffic_source"]
    assert bench.pmc_traffic(samples, "k_correlate")["traffic_measured"] is False
    # ... and nothing is measured inside a profiler or without rocprofv3 (the committed file is quoted then)
    monkeypatch.setenv("ROCP_TOOL_LIBRARIES", "x")
    assert bench.measure_traffic_in_run(1 << 22) is None


def test_m0_guard_catches_a_compiler_written_m0(tmp_path):
    """tools/check_m0.py (run by build()): a write of m0 outside the kernel's own asm blocks inside k_correlate_w64
    fails the check; the asm sites themselves pass"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_m0
    good = tmp_path / "good.s"
    good.write_text("_ZN5gr4pm15k_correlate_w64ILi0EEEvv:\n\t;;#ASMSTART\n\ts_mov_b32 m0, s12\n\ts_nop 0\n\t;;#ASMEND\n"
                    "\tv_pk_fma_f32 v[0:1], v[2:3], v[4:5], v[6:7]\n.Lfunc_end0:\n"
                    "_ZN5gr4pm7k_otherEv:\n\ts_movk_i32 m0, 0x400\n.Lfunc_end1:\n")
    seen, sites, _, _, problems = check_m0.check(str(good))
    assert (seen, sites, problems) == (1, 1, [])
    bad = tmp_path / "bad.s"
    bad.write_text("_ZN5gr4pm15k_correlate_w64ILi0EEEvv:\n\ts_mov_b32 m0, s3\n\t;;#ASMSTART\n\ts_mov_b32 m0, s12\n\t;;#ASMEND\n"
                   ".Lfunc_end0:\n")
    seen, sites, _, _, problems = check_m0.check(str(bad))
    assert seen == 1 and len(problems) == 1 and "compiler-generated" in problems[0]


def test_python_sources_reference_no_undefined_names():
    """Static check of every Python file of the repository: a name a function reads without binding it must exist at
    module level or be a builtin.  (Round 4: a misplaced edit left `if headline and not args...` inside
    bench.selfcheck(), which only runs at N > 1 or under --selfcheck -- nothing on the one-GPU path would have
    noticed the NameError before the driver's scaling run.)"""
    import builtins
    import glob
    import symtable

    def undefined(path):
        top = symtable.symtable(open(path).read(), path, "exec")
        mod = {s.get_name() for s in top.get_symbols() if s.is_assigned() or s.is_imported() or s.is_namespace()}
        mod |= {"__file__", "__name__", "__doc__"}
        bad = []

        def walk(t):
            for c in t.get_children():
                for s in c.get_symbols():
                    if s.is_global() and s.is_referenced() and not s.is_assigned():
                        if s.get_name() not in mod and not hasattr(builtins, s.get_name()):
                            bad.append(f"{os.path.relpath(path, ROOT)}:{c.get_lineno()}: {c.get_name()}() reads {s.get_name()}")
                walk(c)
        walk(top)
        return bad

    files = [os.path.join(ROOT, "bench.py"), os.path.join(ROOT, "__graft_entry__.py")]
    for pat in ("tools/*.py", "apps/*.py", "gr4-packet-modem_amd/*.py", "tests/*.py", "tests/golden/*.py", "oracle/*.py"):
        files += sorted(glob.glob(os.path.join(ROOT, pat)))
    assert len(files) > 40
    bad = [b for f in files for b in undefined(f)]
    assert not bad, "\n".join(bad)
