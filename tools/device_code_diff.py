#!/usr/bin/env python3
"""Is the device code of two builds the same?  One line per kernel of two libraries.

    tools/device_code_diff.py LIB_A LIB_B        (e.g. tools/ab_build.sh HEAD~1, then lib/libcrowdnav_base.so lib/libcrowdnav.so)

Every code object of both libraries is unbundled (as tools/kernel_resources.sh does) and the kernels are paired by name:
    identical        the kernel's bytes and its 64-byte descriptor (.kd) are equal, kernel_code_entry_byte_offset masked (it
                     moves with the kernel's place in the code object)
    allocation-only  the descriptor and the notes (vgpr, agpr, sgpr, both spill counts, scratch, static LDS) are equal, as many
                     instructions not counting s_nop, and the same mnemonic histogram not counting s_nop and s_waitcnt (a vector
                     instruction counted with its constant operands): the same program with other register names or another
                     order of independent instructions
    differs          anything else (a kernel that only one library has included); the histogram delta B - A follows
Exit status 1 if any kernel differs.  Bytes are compared and mnemonics counted; no instruction is looked for.
"""
import collections
import os
import re
import struct
import subprocess
import sys
import tempfile

LLVM = os.environ.get("CN_LLVM_BIN", "/opt/rocm/lib/llvm/bin")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
NOTE_KEYS = ["vgpr_count", "agpr_count", "sgpr_count", "sgpr_spill_count", "vgpr_spill_count", "private_segment_fixed_size",
             "group_segment_fixed_size"]


def code_objects(lib, tmp):
    """The gfx950 code objects of a library, one file per translation unit."""
    fat = os.path.join(tmp, "fat.bin")
    subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, lib], check=True)
    b = open(fat, "rb").read()
    pos = [m.start() for m in re.finditer(re.escape(MAGIC), b)]
    out = []
    for n, p in enumerate(pos):
        bundle = os.path.join(tmp, "bundle%d.bin" % n)
        open(bundle, "wb").write(b[p:pos[n + 1] if n + 1 < len(pos) else len(b)])
        subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--unbundle", "--targets=" + TARGET,
                        "--input=" + bundle, "--output=" + bundle + ".co"], check=True)
        out.append(bundle + ".co")
    return out


def symbols(co):
    """{name: bytes} of every defined FUNC and OBJECT symbol of an ELF64 little-endian code object."""
    b = open(co, "rb").read()
    shoff, = struct.unpack_from("<Q", b, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", b, 0x3A)
    sec = [struct.unpack_from("<IIQQQQIIQQ", b, shoff + i * shentsize) for i in range(shnum)]   # name type flags addr off size link info ..
    symtab = next((s for s in sec if s[1] == 2), None) or next(s for s in sec if s[1] == 11)    # SHT_SYMTAB, else SHT_DYNSYM
    stroff = sec[symtab[6]][4]
    out = {}
    for o in range(symtab[4], symtab[4] + symtab[5], 24):
        name, info, _, shndx, value, size = struct.unpack_from("<IBBHQQ", b, o)
        if (info & 15) not in (1, 2) or shndx == 0 or shndx >= shnum or size == 0 or sec[shndx][1] == 8:   # OBJECT / FUNC, not NOBITS
            continue
        at = sec[shndx][4] + (value - sec[shndx][3])
        out[b[stroff + name:b.index(b"\0", stroff + name)].decode()] = b[at:at + size]
    return out


def notes(co):
    """{kernel: {key: value}} from the code object's metadata note."""
    txt = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    out = {}
    for blk in txt.split(".agpr_count:")[1:]:
        blk = ".agpr_count:" + blk
        get = lambda k: (re.search(r"\." + k + r":\s+(\S+)", blk) or [None, None])[1]
        out[get("name")] = {k: get(k) for k in NOTE_KEYS}
    return out


NUMBER = re.compile(r"^-?(0x[0-9a-f]+|\d+(\.\d+)?)$")


def histograms(co, names):
    """{kernel: Counter of mnemonics} for the named kernels of a code object.  A vector instruction is counted together with its
    constant operands (`v_mul_f32 0x40400000`): registers are an allocation's to choose, an arithmetic constant is the program's."""
    if not names:
        return {}
    txt = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr",
                          "--disassemble-symbols=" + ",".join(sorted(names)), co], check=True, capture_output=True, text=True).stdout
    out, cur = {}, None
    for line in txt.split("\n"):
        m = re.match(r"^(?:[0-9a-f]+ )?<([^>]+)>:", line)
        if m:
            cur = out.setdefault(m.group(1), collections.Counter()) if m.group(1) in names else None
        elif cur is not None and line[:1] in (" ", "\t") and line.strip():
            op, _, args = line.strip().partition(" ")
            consts = [a for a in args.split("//")[0].replace(",", " ").split() if NUMBER.match(a)] if op.startswith("v_") else []
            cur[" ".join([op] + consts)] += 1
    return out


def kernels(lib, tmp):
    """{kernel: (code object, symbol, FUNC bytes, masked descriptor, notes)} over every code object of a library."""
    out = {}
    for n, co in enumerate(code_objects(lib, tmp)):
        sym, nt = symbols(co), notes(co)
        for name, kd in sym.items():
            if name.endswith(".kd") and len(kd) == 64 and name[:-3] in sym:
                k = name[:-3]      # (a kernel of internal linkage may have a namesake in another unit: told apart by the unit's index)
                out[k if k not in out else "%s@unit%d" % (k, n)] = (co, k, sym[k], kd[:16] + bytes(8) + kd[24:], nt.get(k, {}))
    return out


def compare(lib_a, lib_b):
    """[(kernel, class, detail)], sorted by kernel name."""
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
        A, B = kernels(lib_a, ta), kernels(lib_b, tb)
        res = {}
        for k in set(A) | set(B):
            if k not in A or k not in B:
                res[k] = ("differs", "only in %s" % (lib_b if k in B else lib_a))
            elif A[k][2:4] == B[k][2:4]:
                res[k] = ("identical", "")
        rest = [k for k in A if k not in res]
        ha, hb = {}, {}
        for co in set(A[k][0] for k in rest):
            ha.update(((co, s), h) for s, h in histograms(co, set(A[k][1] for k in rest if A[k][0] == co)).items())
        for co in set(B[k][0] for k in rest):
            hb.update(((co, s), h) for s, h in histograms(co, set(B[k][1] for k in rest if B[k][0] == co)).items())
        for k in rest:
            a, b = ha[A[k][:2]], hb[B[k][:2]]
            count = lambda h: sum(v for op, v in h.items() if op != "s_nop")
            core = lambda h: {op: v for op, v in h.items() if op not in ("s_nop", "s_waitcnt")}
            why = []
            if A[k][3] != B[k][3]:
                why.append("descriptor")
            if A[k][4] != B[k][4]:
                why.append("notes " + " ".join("%s %s->%s" % (n, A[k][4].get(n), B[k][4].get(n)) for n in NOTE_KEYS if A[k][4].get(n) != B[k][4].get(n)))
            if count(a) != count(b):
                why.append("instructions %d->%d" % (count(a), count(b)))
            if core(a) != core(b) or count(a) != count(b):
                why.append(" ".join("%s%+d" % (op, b[op] - a[op]) for op in sorted(set(a) | set(b)) if a[op] != b[op]))
            res[k] = ("differs", "; ".join(why)) if why else ("allocation-only", "")
    return [(k,) + res[k] for k in sorted(res)]


def main():
    if len(sys.argv) != 3:
        raise SystemExit(__doc__)
    rows = compare(sys.argv[1], sys.argv[2])
    for k, cls, detail in rows:
        print("%-16s %s%s" % (cls, k, "  [" + detail + "]" if detail else ""))
    n = collections.Counter(cls for _, cls, _ in rows)
    print("# %d kernels: %d identical, %d allocation-only, %d differs" % (len(rows), n["identical"], n["allocation-only"], n["differs"]))
    sys.exit(1 if n["differs"] else 0)


if __name__ == "__main__":
    main()
