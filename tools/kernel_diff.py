"""Do two builds of a translation unit hold the same kernels?  Compares two device-only assemblies
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -mllvm -disable-machine-licm --cuda-device-only -S \
        -o A.s <repo>/chomp_amd/csrc/chomp_capi.hip          (and B.s from the other tree)
    python tools/kernel_diff.py A.s B.s
kernel by kernel: the set of kernel symbols, each kernel's instruction text from its label to its
end (block labels without the function's number, so that the order of instantiation may move) and
its metadata (the fields tools/kernel_regs.py reads, and the kernarg size).  Prints what differs;
exit status 1 if anything does."""
import re, sys
FIELDS = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "private_segment_fixed_size",
          "group_segment_fixed_size", "kernarg_segment_size")


def kernels(path):
    s = open(path).read()
    meta = {}
    for blk in re.findall(r'(- \.agpr_count:.*?\.wavefront_size:\s+\d+)', s, re.S):
        g = lambda k: re.search(r'\.%s:\s+(\d+)' % k, blk)
        meta[re.search(r'\.name:\s+(\S+)', blk).group(1)] = {k: g(k).group(1) if g(k) else '?' for k in FIELDS}
    text = {m.group(1): re.sub(r'\.LBB\d+_', '.LBB_', m.group(2)) for m in re.finditer(
        r'^\t\.type\t(\S+),@function\n\1:[^\n]*\n(.*?)^\.Lfunc_end\d+:', s, re.S | re.M)}
    return meta, text


(ma, ta), (mb, tb) = kernels(sys.argv[1]), kernels(sys.argv[2])
bad = 0
for name in sorted(set(ma) | set(mb)):
    if name not in ma or name not in mb:
        what = "only in " + (sys.argv[1] if name in ma else sys.argv[2])
    else:
        what = ", ".join(["%s %s -> %s" % (k, ma[name][k], mb[name][k]) for k in FIELDS
                          if ma[name][k] != mb[name][k]]
                         + (["instruction text"] if ta.get(name) != tb.get(name) or name not in ta else []))
    if what:
        bad += 1
        print("%s: %s" % (name, what))
print("%d kernels against %d: %s" % (len(ma), len(mb), "%d differ" % bad if bad else "no difference"))
sys.exit(1 if bad else 0)
