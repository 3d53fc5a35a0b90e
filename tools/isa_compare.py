#!/usr/bin/env python3
"""Compares the gfx950 ISA of two builds of this tree, kernel by kernel.

`make` keeps hipcc's -save-temps output of rk_kmer.hip under build/isa_kmer and of rk_classify.hip under build/isa; any other
source can be added with  hipcc --offload-arch=gfx950 -O3 -std=c++17 -save-temps -c <file>  in a directory of its own.  Usage:

    git worktree add /tmp/base <commit> && make -C /tmp/base && make
    python tools/isa_compare.py /tmp/base/build build [--all]

For every *gfx950*.s found under both directories: kernels whose instruction streams are identical (the compiler numbers its branch
labels by function, `.LBB7_3`: that number is masked, so a kernel added before another one in the file does not change it), identical up to the
offsets of scalar loads from the kernel-argument segment (an argument struct changed size), or different (with the
instruction counts, and how many of those differ in scalar code only); and, from the .amdhsa_kernel blocks, every kernel whose VGPR count, SGPR count or scratch bytes moved -- a
branch that adds no instruction to a path can still cost it registers or a spill.  No GPU needed."""
import os, re, sys


def base_name(name):
    """a kernel that gained trailing, defaulted `bool = false` template parameters is still the kernel it was"""
    return re.sub(r"(?:Lb0E)+(?=EEv)", "", name)


def kernels(path):
    out, name, body = {}, None, []
    for line in open(path, errors="replace"):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name, body = base_name(m.group(1)), []
            continue
        if name is None:
            continue
        if line.startswith(".Lfunc_end"):
            out[name], name = body, None
            continue
        t = line.split(";")[0].strip()
        if not t or t.startswith(".") or t.endswith(":"):
            continue
        body.append(re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"\s+", " ", t)))
    return out


def vector_stream(body):
    """the vector, LDS and memory instructions alone, scalar register names masked: what is left when only the scalar code around
    the kernel-argument loads was scheduled differently"""
    keep = ("v_", "ds_", "global_", "buffer_", "flat_", "scratch_")
    return [re.sub(r"\bs\[\d+:\d+\]|\bs\d+\b", "S", x) for x in body if x.startswith(keep) and not x.startswith(("v_writelane", "v_readlane"))]


RES = ("next_free_vgpr", "next_free_sgpr", "private_segment_fixed_size")


def resources(path):
    """kernel -> (VGPRs, SGPRs, scratch bytes) as the compiler recorded them"""
    out, name, cur = {}, None, {}
    for line in open(path, errors="replace"):
        m = re.match(r"^\s*\.amdhsa_kernel (\S+)", line)
        if m:
            name, cur = base_name(m.group(1)), {}
            continue
        if name and line.strip() == ".end_amdhsa_kernel":
            out[name], name = tuple(cur.get(r, 0) for r in RES), None
            continue
        m = re.match(r"^\s*\.amdhsa_(\w+) (\d+)", line)
        if name and m and m.group(1) in RES:
            cur[m.group(1)] = int(m.group(2))
    return out


def loose(body):
    # kernel-argument loads: the base register pair holds the segment address, only the immediate offset moves
    return [re.sub(r"^(s_load_dword\w* \S+ s\[\d+:\d+\],) \S+", r"\1 OFF", re.sub(r"^(s_add_u32 s\d+, s\d+,) 0x[0-9a-f]+$|^(s_add_u32 s\d+, s\d+,) \d+$", r"\1\2 OFF", x)) for x in body]


def main(a, b):
    files = {}
    for root in (a, b):
        for d, _, fs in os.walk(root):
            for f in fs:
                if "gfx950" in f and f.endswith(".s"):
                    files.setdefault(f, {})[root] = os.path.join(d, f)
    for f, where in sorted(files.items()):
        if len(where) != 2:
            continue
        ka, kb = kernels(where[a]), kernels(where[b])
        same = args = vec = 0
        changed = []
        for k in sorted(set(ka) & set(kb)):
            if ka[k] == kb[k]:
                same += 1
            elif loose(ka[k]) == loose(kb[k]):
                args += 1
            else:
                changed.append((k, len(ka[k]), len(kb[k])))
                vec += vector_stream(ka[k]) == vector_stream(kb[k])
        print("%s: %d kernels identical, %d identical up to kernel-argument offsets, %d changed, %d only in one build"
              % (f, same, args, len(changed), len(set(ka) ^ set(kb))))
        if changed:
            g = sorted(100.0 * (nb - na) / na for _, na, nb in changed)
            print("   instruction count of the changed kernels: %+.1f %% .. %+.1f %%, median %+.1f %%" % (g[0], g[-1], g[len(g) // 2]))
            print("   %d of them identical in their vector, LDS and memory instructions (scalar registers masked)" % vec)
        for k, na, nb in changed if "--all" in sys.argv else changed[:5]:
            print("   %6d -> %6d instructions  %s" % (na, nb, k[:110]))
        ra, rb = resources(where[a]), resources(where[b])
        moved = [(k, ra[k], rb[k]) for k in sorted(set(ra) & set(rb)) if ra[k] != rb[k]]
        print("   VGPRs / SGPRs / scratch bytes: %d of %d kernels moved (%d in VGPRs, %d in SGPRs, %d in scratch)"
              % (len(moved), len(set(ra) & set(rb)), sum(x[0] != y[0] for _, x, y in moved), sum(x[1] != y[1] for _, x, y in moved),
                 sum(x[2] != y[2] for _, x, y in moved)))
        for k, x, y in moved if "--all" in sys.argv else moved[:5]:
            print("   %3d/%3d/%4d -> %3d/%3d/%4d  %s" % (x + y + (k[:100],)))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
