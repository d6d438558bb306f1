"""Do two builds of a kernel file hold the same machine code for the kernels a pattern names?
  same_kernels.py OLD.s NEW.s [PATTERN]   (the gfx950 .s files of two `hipcc --save-temps` runs)
PATTERN: a regular expression over the mangled kernel symbols; without one, crc32_kernel.hip's crc32_rows_kernel.
Per kernel: the text from its label to its last s_endpgm (.Lfunc_end) without comments, with symbol
names and the function number of .LBB<n>_<m> labels replaced, hashed, plus its
register, scratch and LDS sizes.  The two multisets must be equal: a refactor
of the kernel's template arguments or of the launch code changes no instruction.
"""
import collections
import hashlib
import re
import sys

SYM = sys.argv[3] if len(sys.argv) > 3 else r"_ZN3lnx17crc32_rows_kernel\w+"
COUNTS = ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")


def kernels(path):
    text = open(path).read()
    # the metadata's entry of each kernel: "  - .agpr_count: ..." to the next one
    meta = {re.search(r"\.name:\s+(\S+)", e).group(1): e for e in re.split(r"^  - (?=\.agpr_count:)", text, flags=re.M)[1:]}
    found = collections.Counter()
    for m in re.finditer(rf"^({SYM}):.*\n((?:.*\n)*?)\.Lfunc_end\d+:", text, flags=re.M):
        body = re.sub(r"\s*;.*", "", m.group(2))
        body = re.sub(r"_Z\w+", "SYM", body)
        body = re.sub(r"\.LBB\d+_", ".LBBn_", body)
        body = "\n".join(l.strip() for l in body.splitlines() if l.strip())
        counts = tuple(int(re.search(rf"\.{c}:\s+(\d+)", meta[m.group(1)]).group(1)) for c in COUNTS)
        found[(hashlib.sha256(body.encode()).hexdigest()[:16], counts)] += 1
    return found


old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
print(f"{sum(old.values())} kernels ({len(old)} distinct) against {sum(new.values())} ({len(new)} distinct)")
for k in sorted((old - new) + (new - old)):
    print(("only old: " if k in old - new else "only new: ") + f"{k[0]} {dict(zip(COUNTS, k[1]))}")
sys.exit(0 if old == new and old else 1)
