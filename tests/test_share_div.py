"""The tiered bills' period shares from one reciprocal (recip_rn, div_by_recip,
share_window in dgen_amd/csrc/dgen_hip.hip): tests/check_share_div.c restates
the FMA sequence and the window on the host and compares every accepted pair
with u / U bit for bit, over the hardware reciprocal's documented error (the
seed cut to 24-26 bits, +-1 in the last kept bit)."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "check_share_div.c")


def test_share_division_equals_the_ieee_quotient(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no C compiler to build tests/check_share_div.c")
    exe = tmp_path / "check_share_div"
    # -ffp-contract=off: the sequence is the source's fma() calls and nothing else
    subprocess.run([cc, "-O2", "-ffp-contract=off", "-fsanitize=undefined", "-fno-sanitize-recover=undefined",
                    "-o", str(exe), SRC, "-lm"], check=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    bad, wbad, total = (int(v) for v in res.stdout.split())
    print(f"pairs x seeds checked {total}, quotient mismatches {bad}, window mistakes {wbad}")
    assert res.returncode == 0 and res.stderr == "", res.stderr[-2000:]
    assert total > 30_000_000
    assert bad == 0 and wbad == 0


def test_the_device_helper_is_the_checked_sequence():
    """The host restatement and the device code are the same operations in the
    same order (text of the three functions, fma spelled __builtin_fma)."""
    hip = open(os.path.join(REPO, "dgen_amd", "csrc", "dgen_hip.hip")).read()
    for line in ("const double e = __builtin_fma(-U, y, 1.0);", "y = __builtin_fma(y, e, y);",
                 "const double q0 = u * y;", "const double r = __builtin_fma(-U, q0, u);",
                 "return __builtin_fma(r, y, q0);", "for (int k = 0; k < 3; k++) {",
                 "U >= 0x1p-256 && hmax < 0x4FF00000u && emin >= -255 && lo32(U) != 0xFFFFFFFFu"):
        assert line in hip, line
    c = open(SRC).read()
    for line in ("const double e = fma(-U, y, 1.0);", "y = fma(y, e, y);", "const double q0 = u * y;",
                 "const double r = fma(-U, q0, u);", "return fma(r, y, q0);", "for (int k = 0; k < 3; k++) {",
                 "U >= 0x1p-256 && hmax < 0x4FF00000u && emin >= -255 && (uint32_t)bits(U) != 0xFFFFFFFFu"):
        assert line in c, line
