"""The VXBA_* environment knobs and the launch seam of voxel-slam_amd/csrc, without a GPU.

  * vxu::env_flag / vxu::env_int (csrc/vxba_env.hpp) through tests/hostmath/launch_knobs_hostcheck.cpp, a host program of its own built with g++: every
    knob's parsing rule on the values below against a table transcribed from the code BEFORE the readers existed (commit bcb82cb; file:line in the
    comments), and the call in csrc that the host program repeats for the knob is looked up in the source, so the table cannot drift from the library;
  * the same program built with the thread sanitizer: eight threads through one cached reader at once;
  * the seam's structure: one file spells the event launch, one the LDS attribute, one getenv.
"""
import os
import re
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "voxel-slam_amd", "csrc")
SRC = os.path.join(HERE, "hostmath", "launch_knobs_hostcheck.cpp")

#          unset  ""  "0" "1" "2" "64" "-3" "x"  "40"   ("40": one more than the rules need, for the one knob whose call site keeps a range)
VALUES = (None, "", "0", "1", "2", "64", "-3", "x", "40")
ON_AT_1 = (0, 0, 0, 1, 0, 0, 0, 0, 0)             # e && e[0] == '1'
OFF_AT_0 = (1, 1, 0, 1, 1, 1, 1, 1, 1)            # !(e && e[0] == '0')
EXPECT = {
    "VXBA_DBG": ON_AT_1,                           # vxba_kernels.hip:1233, 1284, 1321, 1511
    "VXBA_DBG.fused": (0, 0, 0, 1, 1, 0, 0, 0, 0),  # vxba_kernels.hip:1357   ev[0] == '1' || ev[0] == '2'
    "VXBA_LI_TIMING": ON_AT_1,                     # vxba_capi_li.hip:348, 761
    "VXBA_VOXELIZE_WAITS": ON_AT_1,                # vxba_voxelize.hip:402
    "VXBA_K23_PAIR": OFF_AT_0,                     # vxba_kernels.hip:1367
    "VXBA_VOXELIZE_PARTITION": OFF_AT_0,           # vxba_voxelize.hip:600
    "VXBA_VOXELIZE_COMPACT_KEY": OFF_AT_0,         # vxba_voxelize.hip:601
    "VXBA_LIO_DEVICE_EKF": OFF_AT_0,               # vxba_lio.hip:802
    "VXBA_LI_REC_VRAM": OFF_AT_0,                  # vxba_capi_li.hip:370-371
    "options_from_env": OFF_AT_0,                  # vxba_capi_core.hip:230   e[0] == '0' || e[0] == '1' ? e[0] - '0' : dflt, dflt 1 at all four
    "VXBA_K2_HEAD_START": (100, 0, 0, 1, 2, 64, 0, 0, 40),    # vxba_kernels.hip:1234, 1358   atoi, default K2_HEAD_START = 100, negative -> 0
    "VXBA_K2_VPB": (64, 0, 0, 1, 2, 64, -3, 0, 40),           # vxba_capi_core.hip:236-237    atoi, default 64; :238 keeps [32, 64], else 64
    "VXBA_WIDE_NWG": (128, 1, 1, 1, 2, 64, 1, 1, 40),         # vxba_wide.hip:962-963         cap = 128; max(1, atoi)
    "VXBA_MAP_FIX_COMPACT_AT": (0, 0, 0, 1, 2, 64, -3, 0, 40),  # vxba_map.hip:1422-1424      atoll, taken where > 0 (unset: nothing to take)
    "VXBA_SPIN_US": (4000, 0, 0, 1, 2, 64, 0, 0, 40),         # vxba_wait.hpp:19-21           atol, default 4000, negative -> 0
    "VXBA_MAP_DEBUG": (0, 1, 1, 1, 1, 1, 1, 1, 1),            # vxba_map.hip:1532             getenv(...) != nullptr
}
# the reader call of each knob in csrc: (file, the call's text); options_from_env's four knobs share one rule
SITES = {
    "VXBA_DBG": ("vxba_kernels.hip", 'vxu::env_flag("VXBA_DBG", 0, "12")'),
    "VXBA_LI_TIMING": ("vxba_capi_li.hip", 'vxu::env_flag("VXBA_LI_TIMING", 0)'),
    "VXBA_VOXELIZE_WAITS": ("vxba_voxelize.hip", 'vxu::env_flag("VXBA_VOXELIZE_WAITS", 0)'),
    "VXBA_K23_PAIR": ("vxba_kernels.hip", 'vxu::env_flag("VXBA_K23_PAIR", 1)'),
    "VXBA_VOXELIZE_PARTITION": ("vxba_voxelize.hip", 'vxu::env_flag("VXBA_VOXELIZE_PARTITION", 1)'),
    "VXBA_VOXELIZE_COMPACT_KEY": ("vxba_voxelize.hip", 'vxu::env_flag("VXBA_VOXELIZE_COMPACT_KEY", 1)'),
    "VXBA_LIO_DEVICE_EKF": ("vxba_lio.hip", 'vxu::env_flag("VXBA_LIO_DEVICE_EKF", 1)'),
    "VXBA_LI_REC_VRAM": ("vxba_capi_li.hip", 'vxu::env_flag("VXBA_LI_REC_VRAM", 1)'),
    "VXBA_FUSED_SOLVE": ("vxba_capi_core.hip", 'vxu::env_flag("VXBA_FUSED_SOLVE", 1)'),
    "VXBA_SPEC_COLLECTIVE": ("vxba_capi_core.hip", 'vxu::env_flag("VXBA_SPEC_COLLECTIVE", 1)'),
    "VXBA_WIDE_DEVICE_SOLVE": ("vxba_capi_core.hip", 'vxu::env_flag("VXBA_WIDE_DEVICE_SOLVE", 1)'),
    "VXBA_FUSED_SWEEPS": ("vxba_capi_core.hip", 'vxu::env_flag("VXBA_FUSED_SWEEPS", 1)'),
    "VXBA_K2_HEAD_START": ("vxba_kernels.hip", 'vxu::env_int("VXBA_K2_HEAD_START", K2_HEAD_START, 0)'),
    "VXBA_K2_VPB": ("vxba_capi_core.hip", 'vxu::env_int("VXBA_K2_VPB", 64)'),
    "VXBA_WIDE_NWG": ("vxba_wide.hip", 'vxu::env_int("VXBA_WIDE_NWG", 128, 1)'),
    "VXBA_MAP_FIX_COMPACT_AT": ("vxba_map.hip", 'vxu::env_int("VXBA_MAP_FIX_COMPACT_AT", 0)'),
    "VXBA_SPIN_US": ("vxba_wait.hpp", 'vxu::env_int("VXBA_SPIN_US", 4000, 0)'),
    "VXBA_MAP_DEBUG": ("vxba_map.hip", 'vxu::env_flag("VXBA_MAP_DEBUG", 0, nullptr)'),
}


def _read(name):
    with open(os.path.join(CSRC, name)) as fh:
        return fh.read()


def _build(tmp_path, name, *flags):
    cxx = shutil.which("g++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / name)
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pthread", *flags, "-o", exe, SRC], check=True)
    return exe


def _env(value):
    env = {k: v for k, v in os.environ.items() if k != "KNOB"}
    if value is not None:
        env["KNOB"] = value
    return env


def test_every_knob_keeps_its_parsing_rule(tmp_path):
    exe = _build(tmp_path, "launch_knobs_hostcheck")
    for i, value in enumerate(VALUES):
        run = subprocess.run([exe], env=_env(value), capture_output=True, text=True)
        assert run.returncode == 0, run.stdout + run.stderr
        got = dict(line.split() for line in run.stdout.splitlines())
        assert set(got) == set(EXPECT)
        for knob, table in EXPECT.items():
            assert int(got[knob]) == table[i], f"{knob} at {value!r}: {got[knob]}, the code before the readers gave {table[i]}"


def test_the_host_program_repeats_the_calls_of_the_library():
    """Each knob is read in csrc by exactly the call the host program makes for it (with KNOB for the name), and by no other reader call."""
    host = open(SRC).read()
    calls = {}
    for name in sorted(n for n in os.listdir(CSRC) if n.endswith((".hip", ".hpp", ".h"))):
        for m in re.finditer(r'vxu::env_(?:flag|int)\("(VXBA_\w+)"[^()]*\)', _read(name)):
            calls.setdefault(m.group(1), set()).add((name, m.group(0)))
    assert set(calls) == set(SITES)
    for knob, (fname, call) in SITES.items():
        assert calls[knob] == {(fname, call)}, (knob, calls[knob])
        row = "options_from_env" if fname == "vxba_capi_core.hip" and "env_flag" in call else knob
        as_host = call.replace(f'"{knob}"', "KNOB").replace("K2_HEAD_START", "100")
        mark = "const int level" if knob == "VXBA_DBG" else f'"{row} %'      # VXBA_DBG: one read, both spellings derived from it
        line = [ln for ln in host.splitlines() if mark in ln]
        assert line and all(as_host in ln for ln in line), (knob, as_host)


def test_a_cached_reader_under_eight_threads(tmp_path):
    """Thread sanitizer on the stand-alone program: the `static const` of a call site is initialised once while eight threads arrive together."""
    exe = _build(tmp_path, "launch_knobs_tsan", "-fsanitize=thread")
    for value, level in (("1", 1), ("2", 2), (None, 0)):
        run = subprocess.run([exe, "threads"], env=_env(value), capture_output=True, text=True)
        assert run.returncode == 0 and run.stdout.strip() == f"threads ok {level}", run.stdout + run.stderr


def test_the_seam_is_in_one_place():
    src = {n: _read(n) for n in sorted(os.listdir(CSRC)) if n.endswith((".hip", ".hpp", ".h"))}
    assert [n for n, s in src.items() if "hipExtLaunchKernelGGL" in s] == ["vxba_launch.hpp"]
    assert [n for n, s in src.items() if "hipFuncSetAttribute" in s] == ["vxba_launch.hpp"]
    assert [n for n, s in src.items() if "getenv" in s] == ["vxba_env.hpp"]
    assert src["vxba_env.hpp"].count("getenv(") == 2 and src["vxba_launch.hpp"].count("hipFuncSetAttribute(") == 1
    assert not [n for n, s in src.items() if "static int dbg = -1" in s]
    for macro in ("K3_ARGS", "K23_ARGS", "K23_LAUNCH"):
        assert macro not in src["vxba_kernels.hip"]
    assert "k2_voxels_per_block(int" not in src["vxba_kernels.h"]
