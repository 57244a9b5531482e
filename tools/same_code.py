"""Does a change to the device header leave the generated code alone?  (no GPU)

usage: python tools/same_code.py OLD_HEADER [job filter] [--scratch DIR]

Compiles every module of build()'s list (pathtrace.modules.product_jobs(), the
tests/precompile_*.py lists, TEST_DEFINES with their defines and the self-test
module) twice -- with PT_DEVICE_HEADER=OLD_HEADER and with the built-in
header -- into two scratch caches, and compares the .text, .rodata and .note
sections of each pair of code objects: the instructions, the kernel
descriptors and the metadata with the register, scratch and LDS sizes.  One
line per module: identical, or which sections differ, the sizes of .text, how
many disassembly lines differ and whether every kernel still has the same
count of each opcode ("reordered": nothing but that differs).  Exit status 1
if any module is not identical.

The old header of a refactor is `git show <parent>:path-trace_amd/csrc/device/pt_device.h`
written to a scratch file.  The job filter is a list of job numbers and
ranges ("0-8,41"; the product's configurations come first, in
scenes.CONFIGS' order).  --scratch keeps the two caches in DIR, so a second
run compiles only what changed; the default is a temporary directory.

Only chained modules (PT_CHAIN) are generated from the header's PT_CHAIN
regions; every other kind gets the header without them (csrc/devsrc.cpp).  An
old header from before that kind cannot build a chained module: those jobs
are compiled on the new side alone and listed as "new kind".

Bytes and line counts only: which instructions a kernel uses is not looked at."""
import collections
import hashlib
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "path-trace_amd", "csrc", "device", "pt_device.h")
SECTIONS = (".text", ".rodata", ".note")


def _entry():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as entry
    return entry


def _one(k: int) -> None:
    entry = _entry()
    n = len(entry._jobs()) + len(entry._test_defines())
    if k < n:
        entry._compile_job(k)
    else:
        entry._precompile_selftest()


def _llvm(tool: str) -> str:
    rocm = os.environ.get("ROCM_PATH") or "/opt/rocm"
    return os.path.join(rocm, "llvm", "bin", tool)


def _without_chain(text: str) -> str:
    """csrc/devsrc.cpp without_chain: the header as every module kind but the chained one gets it"""
    out, skip = [], False
    for ln in text.splitlines(keepends=True):
        if ln.rstrip("\n") == "#ifdef PT_CHAIN":
            skip = True
        if not skip:
            out.append(ln)
        elif ln.rstrip("\n") == "#endif /* PT_CHAIN */":
            skip = False
    return "".join(out)


def _modules(cache: str, header: str, since: float) -> dict:
    """the code objects this run used (the runtime touches the ones it serves), by their generated
    source without the header's text"""
    text = open(header).read()
    plain = _without_chain(text)
    out = {}
    for f in sorted(os.listdir(cache)):
        hsaco = os.path.join(cache, f[:-4] + ".hsaco")
        if f.endswith(".hip") and os.path.exists(hsaco) and os.path.getmtime(hsaco) >= since:
            src = open(os.path.join(cache, f)).read()
            out[src.replace(text if text in src else plain, "<pt_device.h>", 1)] = f[:-4]
    return out


def _chain_jobs(entry) -> set:
    """the indices of tests/precompile_chain.py's jobs in _jobs(): they precede the inside-zero tail"""
    try:
        import precompile_chain
    except ImportError:
        return set()
    end = len(entry._jobs()) - len(entry._inside_zero_jobs())
    return set(range(end - len(precompile_chain.test_jobs()), end))


def _section(hsaco: str, name: str) -> bytes:
    with tempfile.NamedTemporaryFile() as t:
        subprocess.check_call([_llvm("llvm-objcopy"), "-O", "binary", "--only-section=" + name, hsaco, t.name])
        return open(t.name, "rb").read()


def _disassembly(hsaco: str) -> dict:
    """kernel or function name -> its instructions, addresses and raw bytes stripped"""
    out = subprocess.check_output([_llvm("llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", hsaco],
                                  text=True)
    fns, cur = collections.OrderedDict(), None
    for ln in out.splitlines():
        m = re.match(r"^(?:[0-9a-f]+ )?<(.+)>:$", ln)
        if m:
            cur = fns.setdefault(m.group(1), [])
        elif cur is not None and ln.strip():
            cur.append(re.sub(r"\s*//.*", "", ln).strip())
    return fns


def _compare(old: str, new: str) -> str:
    """'identical', 'reordered' (.text alone differs: the same size and, per kernel, the same count
    of each opcode, so only order and register names) or 'DIFFERS', then the figures"""
    diff = [s for s in SECTIONS if _section(old, s) != _section(new, s)]
    if not diff:
        return "identical"
    msg = "in " + " ".join(diff)
    same_ops = False
    if ".text" in diff:
        a, b = _disassembly(old), _disassembly(new)
        la, lb = sum(a.values(), []), sum(b.values(), [])
        lines = sum(x != y for x, y in zip(la, lb)) + abs(len(la) - len(lb))
        same_ops = list(a) == list(b) and all(
            collections.Counter(i.split()[0] for i in a[f]) == collections.Counter(i.split()[0] for i in b[f])
            for f in a)
        sa, sb = len(_section(old, ".text")), len(_section(new, ".text"))
        msg += "; .text %d -> %d bytes, %d -> %d disassembly lines, %d differ, opcode counts per kernel %s" % (
            sa, sb, len(la), len(lb), lines, "the same" if same_ops else "differ")
        same_ops = same_ops and sa == sb
    return ("reordered; " if diff == [".text"] and same_ops else "DIFFERS; ") + msg


def _label(residual: str) -> str:
    """what tells a module from the others: a hash of its generated text and its defines"""
    pre = residual.split("<pt_device.h>")[0]
    defs = " ".join("%s=%s" % (m.group(1), m.group(2) or "1")
                    for m in re.finditer(r"^#define (PT_\w+) ?(\S*)$", pre, re.M))
    return "%s [%s]" % (hashlib.sha1(residual.encode()).hexdigest()[:8], defs)


def main(argv) -> int:
    if len(argv) >= 2 and argv[0] == "--one":
        _one(int(argv[1]))
        return 0
    scratch = None
    if "--scratch" in argv:
        k = argv.index("--scratch")
        scratch = os.path.abspath(argv[k + 1])
        argv = argv[:k] + argv[k + 2:]
    if not argv or argv[0].startswith("-"):
        print(__doc__)
        return 2
    old_header = os.path.abspath(argv[0])
    sys.path.insert(0, os.path.join(ROOT, "path-trace_amd"))
    import build_ext
    build_ext.build()  # the built-in header is the tree's
    entry = _entry()
    n = len(entry._jobs()) + len(entry._test_defines()) + 1
    picked = list(range(n))
    if len(argv) > 1:
        picked = []
        for part in argv[1].split(","):
            lo, _, hi = part.partition("-")
            picked += range(int(lo), int(hi or lo) + 1)
    tmp = None
    if scratch is None:
        tmp = tempfile.TemporaryDirectory(prefix="same_code_")
        scratch = tmp.name
    new_only = set() if "PT_CHAIN" in open(old_header).read() else _chain_jobs(entry)
    caches = {side: os.path.join(scratch, side) for side in ("old", "new")}
    for c in caches.values():
        os.makedirs(c, exist_ok=True)
    procs, failed, start = [], [], time.time() - 1

    def reap(p):
        if p.wait() != 0:
            failed.append(p.args[-1])
            print(open(p.log).read()[-4000:])
    for k in picked:
        for side in ("old", "new"):
            if side == "old" and k in new_only:
                continue
            env = dict(os.environ, PT_JIT_CACHE=caches[side])
            env.pop("PT_DEVICE_HEADER", None)
            if side == "old":
                env["PT_DEVICE_HEADER"] = old_header
            log = os.path.join(caches[side], "job_%d.log" % k)
            p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--one", str(k)], env=env, cwd=ROOT,
                                 stdout=open(log, "w"), stderr=subprocess.STDOUT)
            p.log = log
            procs.append(p)
            while len(procs) >= 8:  # wait for any one of them
                done = [q for q in procs if q.poll() is not None]
                for q in done:
                    procs.remove(q)
                    reap(q)
                if not done:
                    time.sleep(0.2)
    for p in procs:
        reap(p)
    if failed:
        print("compile jobs failed: %s" % " ".join(failed))
        return 1
    old, new = _modules(caches["old"], old_header, start), _modules(caches["new"], HEADER, start)
    classes = collections.Counter()
    for residual in sorted(set(old) | set(new), key=_label):
        if residual not in old and re.search(r"^#define PT_CHAIN 1$", residual.split("<pt_device.h>")[0], re.M):
            res = "new kind"
        elif residual not in old or residual not in new:
            res = "UNPAIRED (only in the %s cache)" % ("old" if residual in old else "new")
        else:
            res = _compare(os.path.join(caches["old"], old[residual] + ".hsaco"),
                           os.path.join(caches["new"], new[residual] + ".hsaco"))
        classes[res.split(";")[0]] += 1
        print("%s -> %s  %s: %s" % (old.get(residual, "-" * 16), new.get(residual, "-" * 16), _label(residual), res))
    print("%d jobs, %d modules: %s" % (len(picked), sum(classes.values()),
                                       ", ".join("%d %s" % (v, k) for k, v in sorted(classes.items()))))
    return 0 if set(classes) <= {"identical", "new kind"} else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
