"""Static ISA statistics of the C3 fast kernel for device-library variants
(A/B triage on the CPU before a GPU run): size, spills, and every lane-major
generation round instance the kernel holds (one per burst_t variant that has
the round; burst() instantiates up to three variants, and only the reachable
ones under PT_REACH_PRUNE).
usage: python tools/ab/isa_stat.py [header|-] ...  (PT_DEVICE_DEFINES passes through)

Importable: kernel_stats(hsaco) is what tests/test_scene_facts.py checks."""
import collections
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin")
OBJDUMP = os.path.join(LLVM, "llvm-objdump")
READELF = os.path.join(LLVM, "llvm-readelf")
META = "sgpr_spill_count|vgpr_spill_count|vgpr_count|private_segment_fixed_size"


def metadata(hsaco, kernel="pt_render_fast"):
    """the kernel's spill counts, VGPRs and private segment (code-object notes) and its code bytes (symbol size)"""
    notes = subprocess.run([READELF, "--notes", hsaco], capture_output=True, text=True, check=True).stdout
    meta = {}
    cur = None
    for line in notes.splitlines():
        m = re.match(r"\s+\.name:\s+(\S+)", line)
        if m:
            cur = m.group(1)
        m = re.match(r"\s+\.(%s):\s+(\d+)" % META, line)
        if m and cur == kernel:
            meta[m.group(1)] = int(m.group(2))
    syms = subprocess.run([READELF, "-s", hsaco], capture_output=True, text=True, check=True).stdout
    for line in syms.splitlines():
        w = line.split()
        if len(w) >= 8 and w[3] == "FUNC" and w[7] == kernel:
            meta["code_bytes"] = int(w[2])
    return meta


def rounds(lines):
    """The lane-major generation rounds among a kernel's instruction lines.

    A round advances each attempt's 64-bit engine state by the lane jump
    (st = jA * st + jG), which is the only code of the kernel that uses
    v_addc_co_u32_e64: three per attempt, the PT_KATT attempts of one round
    within a few hundred instructions, and rounds of different burst_t
    instances tens of thousands of instructions apart.  So each cluster of
    them is one instance.  The KR0 = false variant adds kR to every attempt's
    direction (w + kR: three adds per attempt, packed in pairs), the KR0 = true
    one does not: at least two v_pk_add_f32 per attempt mark the former (the
    latter keeps one per attempt, from the direction's own arithmetic)."""
    addc = [i for i, l in enumerate(lines) if l.startswith("v_addc_co_u32_e64")]
    clusters = []
    for i in addc:
        if clusters and i - clusters[-1][-1] < 1000:
            clusters[-1].append(i)
        else:
            clusters.append([i])
    out = []
    for cl in clusters:
        a, b = max(0, cl[0] - 120), cl[-1] + 60
        c = collections.Counter(l.split()[0] for l in lines[a:b] if l and not l.endswith(":"))
        attempts = max(1, len(cl) // 3)
        out.append({
            "at": a, "insts": sum(c.values()), "attempts": attempts,
            "readlane": c["v_readlane_b32"], "writelane": c["v_writelane_b32"],
            "scratch": sum(n for o, n in c.items() if o.startswith("scratch_")),
            "valu": sum(n for o, n in c.items() if o.startswith("v_")),
            "pk_add": c["v_pk_add_f32"],
            "variant": "KR0=false (+kR adds)" if c["v_pk_add_f32"] >= 2 * attempts else "KR0=true (no kR)",
        })
    return out


def kernel_stats(hsaco, kernel="pt_render_fast"):
    dis = subprocess.run([OBJDUMP, "-d", "--mcpu=gfx950", hsaco], capture_output=True, text=True, check=True).stdout
    body = re.split(r"^[0-9a-f]+ <[^>]+>:$", dis.split("<%s>:" % kernel)[1], maxsplit=1, flags=re.M)[0]
    lines = [l.split("//")[0].strip() for l in body.splitlines()]
    ops = [l.split()[0] for l in lines if l and not l.endswith(":")]
    c = collections.Counter(ops)
    st = metadata(hsaco, kernel)
    st.update(insts=len(ops), readlane=c["v_readlane_b32"], writelane=c["v_writelane_b32"],
              scratch=sum(n for o, n in c.items() if o.startswith("scratch_")), nop=c["s_nop"],
              getpc=c["s_getpc_b64"], rounds=rounds(lines))
    return st


def main():
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import pathtrace as pt\nfrom pathtrace import scenes\n"
            "print(scenes.CONFIGS[\"C3\"].device_scene().compile(8))\n") % os.path.join(ROOT, "path-trace_amd")
    for h in sys.argv[1:] or ["-"]:
        env = dict(os.environ)
        if h != "-":
            env["PT_DEVICE_HEADER"] = h
        key = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True,
                             text=True).stdout.strip().splitlines()[-1]
        st = kernel_stats(os.path.join(ROOT, "path-trace_amd", "_jit_cache", key + ".hsaco"))
        rs = st.pop("rounds")
        print("%-26s key %s  code bytes %d  insts %d  readlane %d writelane %d scratch %d nop %d getpc %d | "
              "sgpr_spill %d vgpr_spill %d vgprs %d private %d" % (
                  h, key, st["code_bytes"], st["insts"], st["readlane"], st["writelane"], st["scratch"], st["nop"],
                  st["getpc"], st["sgpr_spill_count"], st["vgpr_spill_count"], st["vgpr_count"],
                  st["private_segment_fixed_size"]))
        print("  %d lane-major round instance%s" % (len(rs), "" if len(rs) == 1 else "s"))
        for k, r in enumerate(rs):
            print("  LM round %d at inst %d, %s: %d insts, %d attempts, readlane %d, writelane %d, scratch %d, "
                  "VALU %d, pk_add %d" % (k, r["at"], r["variant"], r["insts"], r["attempts"], r["readlane"],
                                          r["writelane"], r["scratch"], r["valu"], r["pk_add"]))


if __name__ == "__main__":
    main()
