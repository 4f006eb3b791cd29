"""Instruction classes between the workgroup barriers of a kernel, read from `hipcc -S` output.

For every kernel whose (mangled) name contains the given substring: its register figures from the
metadata, then one line per basic block of every barrier-to-barrier interval, with the count of each
instruction class (by mnemonic prefix). The steady-state path of a loop is the sum of the blocks on it.

usage: python tools/asm_intervals.py file.s name-substring [--min N]   (--min: skip blocks with < N instructions)
"""
import re
import sys

CLASSES = ("mfma", "lds_rd", "dma", "vmem", "wait", "salu", "branch", "lane", "valu", "other")


def classify(op, rest):
    if op.startswith("v_mfma") or op.startswith("v_smfma"):
        return "mfma"
    if op.startswith("ds_"):
        return "lds_rd"
    if op.startswith(("buffer_", "global_", "flat_", "scratch_")):
        return "dma" if re.search(r"\blds\b", rest) else "vmem"
    if op in ("s_waitcnt", "s_nop", "s_sleep") or op.startswith("s_waitcnt"):
        return "wait"
    if op.startswith(("s_cbranch", "s_branch")):
        return "branch"
    if op.startswith(("v_readlane", "v_writelane", "v_readfirstlane")):
        return "lane"
    if op.startswith("s_"):
        return "salu"
    if op.startswith("v_"):
        return "valu"
    return "other"


def kernels(text):
    """name -> list of body lines (between `name:` and `s_endpgm`)"""
    out, name, body = {}, None, []
    for line in text.splitlines():
        m = re.match(r"^(_Z\w+):\s*(;.*)?$", line)
        if m and name is None:
            name, body = m.group(1), []
            continue
        if name is not None:
            body.append(line)
            if line.strip().startswith("s_endpgm"):
                out[name] = body
                name = None
    return out


def metadata(text, name):
    m = re.search(r"\.name:\s+" + re.escape(name) + r"\s*\n(.*?)\.wavefront_size", text, re.S)
    keys = ("sgpr_count", "sgpr_spill_count", "vgpr_count", "vgpr_spill_count", "private_segment_fixed_size")
    ent = m.group(1) if m else ""  # the entry's keys are sorted: these all follow .name
    return {k: (re.search(r"\." + k + r":\s+(\d+)", ent) or [None, "?"])[1] for k in keys}


def intervals(body, minimum):
    seg, blocks, label, cnt = 0, [], "(entry)", dict.fromkeys(CLASSES, 0)

    def flush():
        n = sum(cnt.values())
        if n >= minimum:
            blocks.append((seg, label, dict(cnt)))

    for line in body:
        s = line.split(";")[0].strip()
        if not s or s.startswith("."):
            m = re.match(r"^(\.LBB\w+):", s) or re.match(r"^; (%bb\.\d+):", line)  # label | fall-through block
            if m:
                flush()
                label, cnt = m.group(1), dict.fromkeys(CLASSES, 0)
            continue
        op, _, rest = s.partition(" ")
        if op == "s_barrier":
            flush()
            seg += 1
            label, cnt = label + "+", dict.fromkeys(CLASSES, 0)
            continue
        cnt[classify(op, rest)] += 1
    flush()
    return blocks


def main(argv):
    minimum = int(argv[argv.index("--min") + 1]) if "--min" in argv else 1
    text = open(argv[1]).read()
    for name, body in kernels(text).items():
        if argv[2] not in name:
            continue
        print(name)
        print("  " + "  ".join(f"{k}={v}" for k, v in metadata(text, name).items()))
        print("  interval block              " + " ".join(f"{c:>6s}" for c in CLASSES) + "   not load/wait")
        for seg, label, cnt in intervals(body, minimum):
            work = cnt["salu"] + cnt["branch"] + cnt["lane"] + cnt["valu"] + cnt["other"]
            print(f"  {seg:8d} {label:18s} " + " ".join(f"{cnt[c]:6d}" for c in CLASSES) + f"   {work:6d}")


if __name__ == "__main__":
    main(sys.argv)
