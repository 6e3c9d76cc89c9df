"""Fail the build when a kernel spills: reads the -Rpass-analysis=kernel-resource-usage
remarks hipcc wrote for one source (Makefile) and exits 1 if any kernel's ScratchSize is
not 0 (round 5: a spill of 416 bytes per lane in k_tile's walk-queue instantiation made C2
25 % slower without any other sign).  It also exits 1 when a kernel is over its LDS share
(LDS_CAP) or its VGPR budget (VGPR_CAP), or when a key of those tables names no kernel of its
source any more (a renamed kernel would otherwise lose its cap without a sign).  The tables are
keyed by source (the usage file's base name), then by a part of the kernel's mangled name.
Other compiler output is passed through."""
import os
import re
import sys


# k_tile's workgroups per CU by LDS: 3 for tiles of <= 512 positions (NWP 8 / 16), 2 above.
# The share is the largest measured to keep 3: 53,536 bytes ran at 3 per CU, 54,176 (round 6,
# profiles/r06/d1_*, d2_*) and 54,560 (round 5) bytes ran C2 40-47 % slower with no other sign
# (the occupancy remark does not count the CU's reserved LDS or its allocation granules)
LDS_CAP = {"s2c_tile": {"k_tileILi8E": 53536, "k_tileILi16E": 53536, "k_tileILi32E": 81920, "k_tileILi64E": 81920}}
# k_tile_dense<16 | 32 | 64>: five waves per SIMD, i.e. nine two-wave tiles per CU, need at most
# 96 VGPRs.
VGPR_CAP = {"s2c_dense": {"k_tile_denseILi16EE": 96, "k_tile_denseILi32EE": 96, "k_tile_denseILi64EE": 96}}


def main(path):
    name, bad = None, []
    src = os.path.basename(path).split(".")[0]
    vcap, lcap = VGPR_CAP.get(src, {}), LDS_CAP.get(src, {})
    seen = set()   # the keys of vcap / lcap that matched a kernel
    with open(path) as f:
        for ln in f:
            if "remark:" not in ln:
                if not re.match(r"^\s*\d*\s*\|", ln) and "remark" not in ln:   # (the remarks' source context)
                    sys.stderr.write(ln)
                continue
            m = re.search(r"Function Name: (\S+)", ln)
            if m:
                name = m.group(1)
            m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", ln)
            if m and int(m.group(1)) > 0:
                bad.append((name, int(m.group(1))))
            m = re.search(r" VGPRs: (\d+)", ln)
            if m and name:
                hit = {k: cap for k, cap in vcap.items() if k in name}
                seen.update(hit)
                for k, cap in hit.items():
                    if int(m.group(1)) > cap:
                        sys.stderr.write("error: kernel %s takes %s VGPRs, over the %d that keep its waves per SIMD\n"
                                         % (name, m.group(1), cap))
                        bad.append((name, -1))
            m = re.search(r"LDS Size \[bytes/block\]: (\d+)", ln)
            if m and name:
                hit = {k: cap for k, cap in lcap.items() if k in name}
                seen.update(hit)
                for k, cap in hit.items():
                    if int(m.group(1)) > cap:
                        sys.stderr.write("error: kernel %s takes %s bytes of LDS, over its %d-byte share\n"
                                         % (name, m.group(1), cap))
                        bad.append((name, -1))
    for k in sorted(set(vcap) | set(lcap)):
        if k not in seen:
            sys.stderr.write("error: the cap on %s matches no kernel of %s (renamed? update scripts/check_spills.py)\n" % (k, src))
            bad.append((k, -1))
    for n, s in bad:
        if s < 0:
            continue
        sys.stderr.write("error: kernel %s uses %d bytes of scratch per lane (a register spill, or the kernel arguments copied for an out-of-line call)\n" % (n, s))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
