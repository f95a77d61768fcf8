"""Where the built library carries non-temporal accesses (CPU only: the gfx950
code objects of libbsgp.so, disassembled with the ROCm LLVM llvm-objdump).

The stream policy (bsgp_device.hpp "cache policy", BSGP_STREAM_NT) belongs to
the persistent solver's phase functions alone:
* the phase kernels k_dir, k_col, k_ls, k_bb contain no `nt` access;
* where bsgp_persist.hip's default mask is non-zero, its phase functions
  (persist_dir, persist_ls, persist_bb, persist_col_a) contain the `nt` loads
  and stores of the classes the mask names, and persist_col_a still has plain
  16-byte global loads: the transfer function, which never takes a policy.
"""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "beta-sgp_amd", "libbsgp.so")
PERSIST = os.path.join(ROOT, "beta-sgp_amd", "csrc", "bsgp_persist.hip")

O16, O8, W, SR, SC, PJ = 1, 2, 4, 8, 16, 32  # the kNt* bits of bsgp_device.hpp
# per phase function: the classes whose loads / stores it issues
CLASSES = {
    "persist_dir": (O16 | PJ | O8, SR),
    "persist_ls": (O8 | SR | SC, W | SR | SC),
    "persist_bb": (O16 | SR, W),
    "persist_col_a": (SC, SC),
}
NT = re.compile(r"\bglobal_(load|store)\w*\s.*\bnt\b")


def objdump():
    for d in (os.environ.get("ROCM_PATH", ""), "/opt/rocm"):
        p = os.path.join(d, "llvm", "bin", "llvm-objdump") if d else ""
        if p and os.path.exists(p):
            return p
    return shutil.which("llvm-objdump")


def default_mask():
    m = re.search(r"^#define BSGP_STREAM_NT\s+(\d+)", open(PERSIST).read(), re.M)
    return int(m.group(1)) if m else 0


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    """{symbol: disassembly} of the phase kernels and the float64 persistent
    phase functions of namespace bsgp."""
    tool = objdump()
    if tool is None:
        pytest.skip("llvm-objdump not found")
    if not os.path.exists(LIB):
        pytest.skip("libbsgp.so not built")
    import kernel_meta
    want = re.compile(r"^_ZN4bsgp(\d+)(k_dir|k_col|k_ls|k_bb|persist_dir|persist_ls|persist_bb|"
                      r"persist_col_a)I")
    out = {}
    tmp = tmp_path_factory.mktemp("co")
    for n, co in enumerate(kernel_meta.code_objects(LIB)):
        syms = [s for s in kernel_meta._symbol_bytes(co) if want.match(s)]
        if not syms:
            continue
        f = tmp / f"co{n}.elf"
        f.write_bytes(co)
        txt = subprocess.run([tool, "-d", "--disassemble-symbols=" + ",".join(syms), str(f)],
                             check=True, capture_output=True, text=True).stdout
        for part in re.split(r"\n(?=[0-9a-f]+ <)", txt):
            m = re.match(r"[0-9a-f]+ <([^>]+)>:", part)
            if m and m.group(1) in syms:
                out[m.group(1)] = part
    return out


def test_phase_kernels_are_plain(listing):
    ks = [s for s in listing if re.match(r"^_ZN4bsgp\d+k_(dir|col|ls|bb)I", s)]
    assert {re.match(r"^_ZN4bsgp\d+(k_\w+?)I", s).group(1) for s in ks} == \
        {"k_dir", "k_col", "k_ls", "k_bb"}
    for s in ks:
        hit = NT.search(listing[s])
        assert hit is None, (s, hit.group(0))


def test_persistent_phases_carry_the_default_mask(listing):
    mask = default_mask()
    if mask == 0:
        return  # plain build: nothing to find
    for fn, (lbits, sbits) in CLASSES.items():
        # the instantiation of this mask (float64 where the function has a storage type)
        fs = [s for s in listing
              if re.match(rf"^_ZN4bsgp\d+{fn}I", s) and f"Lj{mask}E" in s
              and (fn == "persist_col_a" or "EdL" in s)]
        assert fs, fn
        for s in fs:
            kinds = {m.group(1) for m in NT.finditer(listing[s])}
            if mask & lbits:
                assert "load" in kinds, s
            if mask & sbits:
                assert "store" in kinds, s
            if fn == "persist_col_a":
                plain = [ln for ln in listing[s].splitlines()
                         if re.search(r"\bglobal_load_dwordx4\s", ln) and not NT.search(ln)]
                assert plain, "persist_col_a: no plain 16-byte load left for the TF"
