"""The C-ABI boundary: libkura.so loads, exports every entry point declared in
include/kura.h, and the ctypes mirror of KuraConfig has the C layout.  No
compute calls are made (no GPU here)."""
import ctypes
import importlib
import os
import re
import subprocess
import tempfile

import pytest

from helpers import ROOT

abi = importlib.import_module("dbs-gym_amd.abi")
HEADER = os.path.join(ROOT, "include", "kura.h")


def declared_functions(debug=False):
    """Entry points declared by kura.h (debug=False: without the KURA_DEBUG-only block)."""
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"static inline[^;{]*\{.*?\n\}", "", src, flags=re.S)   # header-only helpers (kura_coupling_of)
    if not debug:
        src = re.sub(r"#ifdef KURA_DEBUG.*?#endif", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(kura_[a-z_0-9]+)\s*\(", src)))


def test_header_declares_the_boundary():
    names = declared_functions()
    for must in ("kura_create", "kura_destroy", "kura_set_coupling", "kura_set_env_params", "kura_set_spectral",
                 "kura_reset", "kura_step", "kura_reward", "kura_get_state", "kura_set_state", "kura_last_error"):
        assert must in names


def test_library_exports_every_declared_symbol():
    if not os.path.exists(abi.LIB_PATH):
        pytest.skip("libkura.so not built (run __graft_entry__.build())")
    out = subprocess.run(["nm", "-D", "--defined-only", abi.LIB_PATH], capture_output=True, text=True, check=True)
    exported = set(re.findall(r"\bT (kura_\w+)", out.stdout))
    missing = [n for n in declared_functions() if n not in exported]
    assert not missing, missing
    assert set(abi._SYMBOLS) <= exported
    # the product library exports kura.h's product entry points and nothing else
    # (no A/B kernels' or debug-build hooks)
    extra = sorted(exported - set(declared_functions()))
    assert not extra, extra


def test_debug_library_exports_the_debug_entry_points():
    dbg = os.path.join(os.path.dirname(abi.LIB_PATH), "libkura_debug.so")
    if not os.path.exists(dbg):
        pytest.skip("libkura_debug.so not built")
    out = subprocess.run(["nm", "-D", "--defined-only", dbg], capture_output=True, text=True, check=True)
    exported = set(re.findall(r"\bT (kura_\w+)", out.stdout))
    assert set(declared_functions(debug=True)) <= exported


def test_library_loads_and_reports_version():
    if not os.path.exists(abi.LIB_PATH):
        pytest.skip("libkura.so not built")
    lib = abi.load_library()
    assert lib.kura_abi_version() == abi.KURA_ABI_VERSION


def test_missing_library_fails_loudly(tmp_path):
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        abi.load_library(str(tmp_path / "nope.so"))


def test_config_struct_layout_matches_c():
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "kura.h"
#define P(f) printf(#f " %zu\n", offsetof(KuraConfig, f));
int main(void) {
  printf("sizeof %zu\n", sizeof(KuraConfig));
  P(abi_version) P(n_osc) P(bins) P(padlen) P(part_osc) P(coupling) P(reserved_i) P(dt) P(transient_len) P(dbs_hi)
  P(bw_b) P(bw_zi)
  P(rtol) P(kn) P(dt0) P(reserved_f)
  return 0;
}
'''
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "l.c")
        open(c, "w").write(prog)
        exe = os.path.join(d, "l")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        lines = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    got = dict(l.split() for l in lines if l)
    assert int(got["sizeof"]) == ctypes.sizeof(abi.KuraConfig)
    for f, off in got.items():
        if f != "sizeof":
            assert getattr(abi.KuraConfig, f).offset == int(off), f


# Build switches of settled experiments ("Retired build
# switches"): their code is deleted, and a command line that still passes one
# must fail instead of building the product under a variant's name.
RETIRED_SWITCHES = ["KURA_EXP_ALPHA", "KURA_EXP_ORDER", "KURA_EXP_NO_B1", "KURA_EXP_NO_B2", "KURA_SPLIT_SCALAR",
                    "KURA_SI_PACKED", "KURA_GROUPSUM_ATOMIC", "KURA_FUSED_ERR", "KURA_SAVE_PACKED",
                    "KURA_SOLVE_INLINE", "KURA_RESET_DEDUP", "KURA_REC_LD_AUX", "KURA_REC_ST_AUX", "KURA_BITSEL"]


def _preprocess_kernels(*defines):
    import __graft_entry__ as ge
    if not os.path.exists(ge.HIPCC):
        pytest.skip("no hipcc")
    return subprocess.run([ge.HIPCC, *ge.HIP_FLAGS, *defines, "-E", "-o", os.devnull,
                           os.path.join(ge.CSRC, "kura_kernels.hip")], capture_output=True, text=True)


def test_kernel_source_preprocesses_plain():
    r = _preprocess_kernels()
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("macro", RETIRED_SWITCHES)
def test_retired_build_switch_is_an_error(macro):
    r = _preprocess_kernels(f"-D{macro}=1")
    assert r.returncode != 0
    # the #error's own text, not just the echoed command line
    msg = [ln for ln in r.stderr.splitlines() if "error:" in ln and "retired build switch" in ln]
    assert msg and macro in msg[0], r.stderr


def test_metric_entry_points_reject_null_handle():
    """Argument checks run before any HIP call: a null handle is
    KURA_E_INVALID (-1) for the episode-metric entry points, no GPU needed."""
    if not os.path.exists(abi.LIB_PATH):
        pytest.skip("libkura.so not built")
    lib = abi.load_library()
    assert lib.kura_envelope_stats(None, None, None, 16, 1, None, None) == -1
    assert lib.kura_episode_envelope_stats(None, None, None, None) == -1
    assert lib.kura_psd_bbpow(None, None, None, 16, 1, 5e-4, 12.5, 21.0, None, None) == -1
    assert lib.kura_episode_bbpow(None, None, 5e-4, 12.5, 21.0, None, None) == -1


def test_version_1_config_is_rejected():
    """the coupling field reuses version 1's reserved slot (0 = AUTO
    = BF16X3), so a version-1 config is refused with KURA_E_INVALID before any
    HIP call, naming the field to choose."""
    if not os.path.exists(abi.LIB_PATH):
        pytest.skip("libkura.so not built")
    assert abi.KURA_ABI_VERSION == 2
    lib = abi.load_library()
    sim = importlib.import_module("dbs-gym_amd.sim")
    kura = importlib.import_module("dbs-gym_amd")
    cfg = sim.make_config(kura.reference_params("env0"), 4, reward_func="bbpow_action")
    assert cfg.abi_version == 2
    cfg.abi_version = 1
    h = ctypes.c_void_p()
    assert lib.kura_create(ctypes.byref(cfg), 0, ctypes.byref(h)) == -1   # KURA_E_INVALID
    msg = lib.kura_last_error().decode()
    assert "abi_version 1 != 2" in msg and "coupling" in msg
