"""Static counts per kernel from the device assembly `hipcc --save-temps` leaves (*-hip-amdgcn-amd-amdhsa-gfx950.s): VGPRs, spilled
registers, scratch and LDS bytes from the kernel's metadata, and from its text the numbers of VALU instructions, `s_nop`
(with the wait states they add up to), `s_cbranch` and `v_cndmask`. For comparing two builds of the same kernels.
usage: python tools/isa_counts.py FILE.s [substring of a demangled kernel name ...]"""
import re
import subprocess
import sys


def kernels(path):
    text = open(path).read()
    meta = {}
    md = text[text.index("amdhsa.kernels:"):] if "amdhsa.kernels:" in text else ""
    for e in re.split(r"\n  - \.", md)[1:]:  # one list entry per kernel
        m = re.search(r"\n    \.name:\s+(\S+)", e)
        g = lambda k: int((re.search(r"\." + k + r":\s+(\d+)", e) or [0, 0])[1])
        if m:
            meta[m.group(1)] = dict(vgpr=g("vgpr_count"), spill=g("vgpr_spill_count"), scratch=g("private_segment_fixed_size"), lds=g("group_segment_fixed_size"))
    rows = []
    for sym, m in meta.items():
        body = re.search(r"^%s:[^\n]*\n(.*?)^\s+s_endpgm" % re.escape(sym), text, re.S | re.M)
        if not body:
            continue
        ins = [l.split(";")[0].split() for l in body.group(1).split("\n")]
        ins = [t for t in ins if t and not t[0].endswith(":") and not t[0].startswith(".")]
        nops = [int(t[1], 0) + 1 for t in ins if t[0] == "s_nop"]
        rows.append(dict(m, symbol=sym, valu=sum(t[0].startswith("v_") for t in ins), s_nop=len(nops), nop_states=sum(nops),
                         branch=sum(t[0].startswith("s_cbranch") for t in ins), cndmask=sum(t[0].startswith("v_cndmask") for t in ins)))
    names = subprocess.run(["c++filt"], input="\n".join(r["symbol"] for r in rows), capture_output=True, text=True).stdout.split("\n")
    for r, n in zip(rows, names):
        r["name"] = re.sub(r"\(.*$", "", n)
    return rows


if __name__ == "__main__":
    pats = sys.argv[2:]
    for r in kernels(sys.argv[1]):
        if not pats or any(p in r["name"] for p in pats):
            print("%-70s vgpr %3d spill %3d scratch %4d lds %6d | valu %6d s_nop %4d (%4d states) s_cbranch %4d v_cndmask %4d"
                  % (r["name"][-70:], r["vgpr"], r["spill"], r["scratch"], r["lds"], r["valu"], r["s_nop"], r["nop_states"], r["branch"], r["cndmask"]))
