"""Per-kernel register / spill / scratch metadata of the built gfx950 code
objects, read straight from a linked library's (or object's) .hip_fatbin
section: clang offload bundles -> the gfx950 ELF -> its AMDGPU metadata note
(msgpack).  No recompilation, no GPU.

    python3 tools/kernel_meta.py [beta-sgp_amd/libbsgp.so]

prints one line per kernel: VGPRs, AGPRs, VGPR spills, SGPR spills, private
segment bytes (scratch per lane), LDS bytes.  tests/test_regbudget.py holds the
allow-list these must stay within.

    python3 tools/kernel_meta.py --diff OLD NEW

compares two builds (objects or libraries) code object by code object (paired
by the kernels they hold, not by position: the link order follows the file
names of csrc/): the digests of .text and .rodata, and per kernel symbol whether its bytes in .text
and its metadata are equal (likewise the bytes of the device functions the
kernels call), plus the kernels on one side only.  Exit status 0 when every
kernel and function present on both sides is identical.  Bytes and sizes only:
a kernel whose code is unchanged still differs where the unit's layout moved
(PC-relative offsets into .rodata, when other kernels left the unit).  The
evidence that a refactor of the kernel headers left the device code alone.
"""
import hashlib
import struct
import sys

import msgpack

_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def _section_hdr(elf, name):
    """Header (sh_name, type, flags, addr, offset, size, ...) of section `name`
    of a 64-bit little-endian ELF image."""
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", elf, 0x3A)
    def hdr(i):
        return struct.unpack_from("<IIQQQQIIQQ", elf, shoff + i * shentsize)
    strtab = hdr(shstrndx)
    for i in range(shnum):
        h = hdr(i)
        nm = elf[strtab[4] + h[0]:elf.index(b"\0", strtab[4] + h[0])].decode()
        if nm == name:
            return h
    return None


def _section(elf, name):
    """Bytes of section `name`."""
    h = _section_hdr(elf, name)
    return None if h is None else elf[h[4]:h[4] + h[5]]


def _notes(elf):
    """(name, type, desc) of every note of the ELF's .note section."""
    sec = _section(elf, ".note")
    out, o = [], 0
    while sec is not None and o + 12 <= len(sec):
        namesz, descsz, typ = struct.unpack_from("<III", sec, o)
        o += 12
        name = sec[o:o + namesz].rstrip(b"\0").decode()
        o += (namesz + 3) & ~3
        out.append((name, typ, sec[o:o + descsz]))
        o += (descsz + 3) & ~3
    return out


def code_objects(path, arch="gfx950"):
    """Every `arch` code object ELF in the file's offload bundles."""
    data = open(path, "rb").read()
    fb = _section(data, ".hip_fatbin") if data[:4] == b"\x7fELF" else data
    if fb is None:
        return []
    objs, pos = [], fb.find(_MAGIC)
    while pos >= 0:
        n, = struct.unpack_from("<Q", fb, pos + len(_MAGIC))
        o = pos + len(_MAGIC) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", fb, o)
            triple = fb[o + 24:o + 24 + tlen].decode()
            o += 24 + tlen
            if triple.endswith(arch):
                objs.append(fb[pos + off:pos + off + size])
        pos = fb.find(_MAGIC, pos + 1)
    return objs


def _kernels_of(co):
    """{kernel symbol: metadata dict} of one code object."""
    res = {}
    for name, typ, desc in _notes(co):
        if name != "AMDGPU" or typ != 32:  # NT_AMDGPU_METADATA
            continue
        meta = msgpack.unpackb(desc, raw=False)
        for k in meta.get("amdhsa.kernels", []):
            res[k[".name"]] = {
                "vgpr": k.get(".vgpr_count"),
                "agpr": k.get(".agpr_count", 0),
                "vgpr_spill": k.get(".vgpr_spill_count", 0),
                "sgpr_spill": k.get(".sgpr_spill_count", 0),
                "private": k.get(".private_segment_fixed_size", 0),
                "lds": k.get(".group_segment_fixed_size", 0),
                "dyn_stack": k.get(".uses_dynamic_stack", False),
            }
    return res


def kernels(path, arch="gfx950"):
    """{kernel symbol: metadata dict} over every code object of the file."""
    res = {}
    for co in code_objects(path, arch):
        res.update(_kernels_of(co))
    return res


def _symbol_bytes(co):
    """{symbol: its bytes in .text} (st_value, st_size of .symtab) of one code object."""
    sym, strs, text = _section(co, ".symtab"), _section(co, ".strtab"), _section_hdr(co, ".text")
    res = {}
    for o in range(0, len(sym or b""), 24):
        nm, _info, _other, _shndx, value, size = struct.unpack_from("<IBBHQQ", sym, o)
        if size and text[3] <= value and value + size <= text[3] + text[5]:
            off = text[4] + value - text[3]
            res[strs[nm:strs.index(b"\0", nm)].decode()] = co[off:off + size]
    return res


def diff(old, new, arch="gfx950"):
    """Print the comparison of two builds; True when no common kernel differs."""
    a, b = code_objects(old, arch), code_objects(new, arch)
    same = len(a) == len(b)
    print(f"code objects: {len(a)} / {len(b)}")
    # each old code object with the new one that shares the most kernels with it
    rest, pairs = list(b), []
    for x in a:
        kx = set(_kernels_of(x))
        y = max(rest, key=lambda c: len(kx & set(_kernels_of(c))), default=None)
        if y is None or not kx & set(_kernels_of(y)):
            same = False
            print(f"no counterpart of the code object holding {sorted(kx)[:1]}")
            continue
        rest.remove(y)
        pairs.append((x, y))
    for i, (x, y) in enumerate(pairs):
        for sec in (".text", ".rodata"):
            dx, dy = (hashlib.sha256(_section(c, sec) or b"").hexdigest()[:16] for c in (x, y))
            print(f"[{i}] {sec:8s} {dx} {dy} {'equal' if dx == dy else 'DIFFERENT'}")
        (kx, bx), (ky, by) = ((_kernels_of(c), _symbol_bytes(c)) for c in (x, y))
        bad = [k for k in kx if k in ky and (kx[k] != ky[k] or bx.get(k) != by.get(k))]
        same = same and not bad
        print(f"[{i}] kernels {len(kx)} / {len(ky)}, {len(set(kx) & set(ky)) - len(bad)} identical")
        for k in bad:
            p, q = bx.get(k, b""), by.get(k, b"")
            n = sum(u != v for u, v in zip(p, q)) if len(p) == len(q) else -1
            print(f"[{i}]   differs: {k}: {len(p)} / {len(q)} bytes, "
                  f"{n if n >= 0 else 'all'} differ, metadata {'equal' if kx[k] == ky[k] else 'DIFFERENT'}")
        # (the device functions kernels call, e.g. the persistent solver's phases)
        for f in sorted(s for s in bx if s not in kx and s in by and bx[s] != by[s]):
            same = False
            print(f"[{i}]   differs (device function): {f}")
        for tag, ks in (("only in OLD", sorted(set(kx) - set(ky))),
                        ("only in NEW", sorted(set(ky) - set(kx)))):
            for k in ks:
                print(f"[{i}]   {tag}: {k}")
    return same


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--diff":
        sys.exit(0 if diff(sys.argv[2], sys.argv[3]) else 1)
    lib = sys.argv[1] if len(sys.argv) > 1 else "beta-sgp_amd/libbsgp.so"
    for name, m in sorted(kernels(lib).items()):
        print(f"{name[:90]:90s} vgpr={m['vgpr']:3d} spill={m['vgpr_spill']:3d} "
              f"sspill={m['sgpr_spill']:3d} scratch={m['private']:4d} dyn={int(m['dyn_stack'])}")
