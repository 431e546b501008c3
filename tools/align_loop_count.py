"""Static counts of the alignment unit's gfx950 assembly (make -C pl-svo_amd/csrc align_kernels.s).

  python tools/align_loop_count.py pl-svo_amd/csrc/align_kernels.s [other.s]

Per align_fused_kernel<T>: VGPRs, scratch bytes, and the ROUND LOOP of the fused pass -- the shortest loop at depth 4 or more that holds at
least ten dword loads from global memory (the window loads of stage B; the set-up's record loop sits at depth 2): the instructions from its header label to the last branch back to that label,
and among them the sign extensions (v_ashrrev_i32), the 64-bit address adds (v_lshl_add_u64) and the exec-mask saves (s_and_saveexec_b64).
With a second file: per instantiation, whether the two instruction streams are equal once register numbers, label numbers and
comments are taken out (register-allocation noise), and the first lines that differ."""
import re
import sys


def functions(path):
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"^(_ZN9plsvo_hip18align_fused_kernelILi(\d+)EEE\w+):", line)
        if m:
            name, body = int(m.group(2)), []
            continue
        if name is not None:
            if line.startswith(".Lfunc_end"):
                out[name] = body
                name = None
            else:
                body.append(line.rstrip("\n"))
    meta = {}
    cur = None
    for line in open(path):
        m = re.match(r"\s+\.name:\s+_ZN9plsvo_hip18align_fused_kernelILi(\d+)EEE", line)
        if m:
            cur = int(m.group(1))
            meta[cur] = {}
        m = re.match(r"\s+\.(vgpr_count|private_segment_fixed_size|vgpr_spill_count):\s+(\d+)", line)
        if m and cur is not None:
            meta[cur][m.group(1)] = int(m.group(2))
        if re.match(r"\s+\.name:", line) and "align_fused_kernel" not in line:
            cur = None
    return out, meta


def is_instr(line):
    s = line.split(";")[0].strip()
    return bool(s) and not s.endswith(":") and not s.startswith(".")


def round_loop(body):
    best = None
    for i, line in enumerate(body):
        m = re.match(r"^(\.LBB\d+_\d+):", line)
        if not m:
            continue
        # the label's comment block: "Parent Loop ..." lines, then "=> This Loop Header: Depth=N"
        k, head = i, None
        while k < len(body) and (k == i or body[k].strip().startswith(";")):
            head = head or re.search(r"This Loop Header: Depth=(\d+)", body[k])
            k += 1
        if not head:
            continue
        label, depth = m.group(1), int(head.group(1))
        last = None
        for j in range(i + 1, len(body)):
            s = body[j].split(";")[0]
            if re.search(r"\b(s_cbranch\w+|s_branch)\s+" + re.escape(label) + r"\b", s):
                last = j
        if last is None:
            continue
        ins = [l.split(";")[0].strip() for l in body[i + 1:last + 1] if is_instr(l)]
        loads = sum(1 for l in ins if l.startswith("global_load_dword "))
        if depth >= 4 and loads >= 10 and (best is None or len(ins) < best["n"]):   # the ten window loads: the shortest loop that holds them
            best = dict(label=label, depth=depth, n=len(ins), loads=loads, ashr=sum(l.startswith("v_ashrrev_i32") for l in ins),
                        add64=sum(l.startswith("v_lshl_add_u64") for l in ins), saveexec=sum(l.startswith("s_and_saveexec_b64") for l in ins))
    return best


def normalised(body):
    out = []
    for l in body:
        if not is_instr(l):
            continue
        s = l.split(";")[0].strip()
        s = re.sub(r"\b([vsa])\[\d+:\d+\]", r"\1[]", s)
        s = re.sub(r"\b([vsa])\d+\b", r"\1", s)
        s = re.sub(r"\.LBB\d+_\d+", ".L", s)
        out.append(s)
    return out


def main():
    fa, ma = functions(sys.argv[1])
    for T in sorted(fa):
        r = round_loop(fa[T])
        if r is None:   # (no loop with ten separate dword window loads: the row-major shapes request a window row otherwise)
            print(f"<{T}>: VGPRs {ma[T].get('vgpr_count')}, scratch {ma[T].get('private_segment_fixed_size')} B, spilled VGPRs {ma[T].get('vgpr_spill_count')}; "
                  f"no loop with the ten dword window loads; function {sum(is_instr(l) for l in fa[T])} instructions")
            continue
        print(f"<{T}>: VGPRs {ma[T].get('vgpr_count')}, scratch {ma[T].get('private_segment_fixed_size')} B, spilled VGPRs {ma[T].get('vgpr_spill_count')}; "
              f"round loop {r['label']} depth {r['depth']}: {r['n']} instructions, {r['loads']} global dword loads, v_ashrrev_i32 {r['ashr']}, "
              f"v_lshl_add_u64 {r['add64']}, s_and_saveexec_b64 {r['saveexec']}; function {sum(is_instr(l) for l in fa[T])} instructions")
    if len(sys.argv) > 2:
        fb, _ = functions(sys.argv[2])
        for T in sorted(fa):
            a, b = normalised(fa[T]), normalised(fb[T])
            if a == b:
                print(f"<{T}>: instruction streams equal ({len(a)} instructions)")
            else:
                k = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
                print(f"<{T}>: streams differ: {len(a)} / {len(b)} instructions, first difference at {k}: {a[k:k + 2]} / {b[k:k + 2]}")


if __name__ == "__main__":
    main()
