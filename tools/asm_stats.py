"""Static instruction mix of one kernel in a device-assembly file (make asm UNIT=...).

    python tools/asm_stats.py opticalflow3d_dev_amd/csrc/kt_grad3-gfx950.s k_grad_xyz_cItdLi6ELi2E [--dump]

Counts per class (VALU fp64 / other VALU, SALU, LDS, VMEM, branches, waits) over the function body,
and the resource lines (VGPRs, SGPRs, LDS, scratch).  --dump prints the body.

    python tools/asm_stats.py NEW.s --table [--against OLD.s]

One line per kernel of the file: VGPRs, AGPRs, SGPRs, scratch bytes per lane, static LDS, occupancy
and instruction count; with --against, whether the other file's kernel of the same name has the
same resources and the same instruction stream (exit status 1 if names or resources differ)."""
import hashlib
import os
import re
import sys
from collections import Counter


def body(path, key):
    lines = open(path).read().splitlines()
    start = None
    for i, l in enumerate(lines):
        if start is None and re.match(r"^_Z\S*" + re.escape(key) + r"\S*:", l):
            start = i
        elif start is not None and l.startswith(".Lfunc_end"):
            return lines[start:i], lines[i:i + 120]
    raise SystemExit(f"{key}: not found in {path}")


def classify(op):
    if op.startswith("v_") and "f64" in op:
        return "valu_f64"
    if op.startswith(("v_mfma", "v_smfmac")):
        return "mfma"
    if op.startswith("v_"):
        return "valu_other"
    if op.startswith("s_waitcnt") or op.startswith("s_barrier"):
        return "wait/barrier"
    if op.startswith(("s_cbranch", "s_branch")):
        return "branch"
    if op.startswith(("s_load", "s_buffer_load")):
        return "smem"
    if op.startswith("s_"):
        return "salu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("buffer_", "global_", "flat_")):
        return "vmem"
    return "other"


RES = (("vgpr", "NumVgprs"), ("agpr", "NumAgprs"), ("sgpr", "TotalNumSgprs"), ("scratch", "ScratchSize"),
       ("lds", "LDSByteSize"), ("occ", "Occupancy"))


def kernels(path):
    """Every kernel of the file: name -> (resources, sha1 of its instruction stream).  The stream is
    the function body with comments, directives and blank lines dropped and the per-function
    number taken out of local labels, so it does not depend on the order of emission."""
    out, name, stream = {}, None, []
    lines = open(path).read().splitlines()
    for i, l in enumerate(lines):
        if name is None:
            m = re.match(r"^(_Z\S+):", l)
            if m:
                name, stream = m.group(1), []
        elif l.startswith(".Lfunc_end"):
            info = "\n".join(lines[i:i + 60])
            if "; Kernel info:" in info:
                res = tuple(int(re.search(r"; %s: (\d+)" % k, info).group(1)) for _, k in RES)
                out[name] = (res, hashlib.sha1("\n".join(stream).encode()).hexdigest()[:12], len(stream))
            name = None
        else:
            s = l.split(";")[0].strip()
            if s and (not s.startswith(".") or s.startswith(".LBB")):
                stream.append(re.sub(r"\.LBB\d+_", ".LBB_", s))
    return out


def short(name):
    """A mangled kernel name without the anonymous-namespace prefix and the argument list: the
    kernel and its template arguments as the compiler spells them."""
    return re.sub(r"EEv\w*$", "E", re.sub(r"^_ZN12_GLOBAL__N_1\d\d(?=k_)", "", name))


def table(path, against=None):
    """One line per kernel; with `against`, whether the other file's kernel of the same name has
    the same resources and instruction stream, and a summary line."""
    a = kernels(path)
    b = kernels(against) if against else None
    cols = [c for c, _ in RES]
    print("kernel\t" + "\t".join(cols) + "\tinstructions" + ("\tsame_resources\tsame_stream" if b else ""))
    nres = nstream = 0
    for k in sorted(a):
        res, h, n = a[k]
        row = [short(k)] + [str(v) for v in res] + [str(n)]
        if b is not None:
            same_r, same_s = k in b and b[k][0] == res, k in b and b[k][1] == h
            nres += same_r
            nstream += same_s
            row += ["yes" if same_r else "NO " + str(b.get(k, ("missing",))[0]), "yes" if same_s else "NO"]
        print("\t".join(row))
    if b is not None:
        print(f"# {len(a)} kernels, {len(b)} in {os.path.basename(against)}; same names: {sorted(a) == sorted(b)}; "
              f"same resources: {nres}; same instruction stream: {nstream}; "
              f"with scratch: {sum(1 for r, _, _ in a.values() if r[3])}")
        return sorted(a) == sorted(b) and nres == len(a)
    return True


def main():
    if "--table" in sys.argv:
        i = sys.argv.index("--against") if "--against" in sys.argv else 0
        raise SystemExit(0 if table(sys.argv[1], sys.argv[i + 1] if i else None) else 1)
    path, key = sys.argv[1], sys.argv[2]
    b, tail = body(path, key)
    ops = Counter()
    names = Counter()
    for l in b:
        s = l.strip()
        if not s or s.startswith((";", ".", "_")) or s.endswith(":"):
            continue
        op = s.split()[0]
        ops[classify(op)] += 1
        names[op] += 1
    print(" ".join(f"{k}={v}" for k, v in sorted(ops.items())))
    print("top:", ", ".join(f"{k} {v}" for k, v in names.most_common(30)))
    for l in tail:
        if re.search(r"num_vgpr|numbered_sgpr|private_seg_size|group_segment|; (NumVgprs|Occupancy|ScratchSize|LDSByteSize)", l):
            print(l.strip())
    if "--dump" in sys.argv:
        print("\n".join(b))


if __name__ == "__main__":
    main()
