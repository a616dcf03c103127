"""Static instruction counts of the conv7 / bwd7 kernel family ("Round 9"): compiles csrc/conv7.hip and csrc/bwd6.hip
to gfx950 assembly (device side only) and prints, per conv7_kernel / bwd7_kernel instantiation, total instructions, MFMA, SALU,
v_readlane + v_writelane, s_mul*, LDS-DMA issues, and from the code-object metadata SGPR spills, VGPRs, scratch bytes and waves per SIMD.
    python tools/isa_counts.py [--all]        (--all: every kernel of the two files)"""
import os, re, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "heterogeneous-moe-for-diffusion-models_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
NOT_SALU = ("s_waitcnt", "s_barrier", "s_nop", "s_load", "s_buffer_load", "s_endpgm", "s_branch", "s_cbranch", "s_sleep", "s_setprio", "s_code_end")


def demangle(names):
    """kernel<integer template arguments> from the Itanium name (enough for this family: int / bool arguments only)"""
    out = {}
    for n in names:
        m = re.search(r"\d+([a-z]\w*?_kernel\w*?)I((?:L[a-z]\d+E)+)E", n)
        out[n] = m.group(1) + "<" + ",".join(re.findall(r"L[a-z](\d+)E", m.group(2))) + ">" if m else n
    return out


def compile_asm(srcs, d):
    """device-side assembly of each source (in parallel) -> {src: text}"""
    procs = {src: subprocess.Popen([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-munsafe-fp-atomics", "--cuda-device-only", "-S",
                                    f"-I{CSRC}", f"-I{os.path.join(ROOT, 'include')}", os.path.join(CSRC, src), "-o", os.path.join(d, src + ".s")],
                                   stderr=subprocess.DEVNULL) for src in srcs}
    for src, p in procs.items():
        if p.wait():
            raise RuntimeError(f"{src}: hipcc failed")
    return {src: open(os.path.join(d, src + ".s")).read() for src in srcs}


def counts(text):
    rows = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end", text, flags=re.S | re.M):
        name, body = m.group(1), m.group(2)
        ins = [l.split()[0] for l in body.split("\n") if l.startswith("\t") and not l.startswith("\t.") and not l.startswith("\t;") and l.strip()]
        rows[name] = dict(
            instr=len(ins), mfma=sum(i.startswith("v_mfma") for i in ins),
            salu=sum(i.startswith("s_") and not i.startswith(NOT_SALU) for i in ins),
            lanes=sum(i.startswith(("v_readlane", "v_writelane")) for i in ins),
            smul=sum(i.startswith("s_mul") for i in ins), dma=sum(i.startswith("buffer_load") and " lds" in l for i, l in
                                                                  ((l.split()[0], l) for l in body.split("\n") if l.startswith("\tbuffer_load"))))
    for m in re.finditer(r"\.name:\s+(_Z\w+)\n(.*?)\.wavefront_size", text, flags=re.S):
        if m.group(1) in rows:
            md = m.group(2)
            g = lambda k: int(re.search(rf"\.{k}:\s+(\d+)", md).group(1))
            rows[m.group(1)].update(spill=g("sgpr_spill_count"), vgpr=g("vgpr_count"), scratch=g("private_segment_fixed_size"))
    for m in re.finditer(r"^\s*\.amdhsa_kernel (_Z\w+)\n(.*?)\.end_amdhsa_kernel", text, flags=re.S | re.M):
        if m.group(1) in rows:
            acc = re.search(r"\.amdhsa_accum_offset (\d+)", m.group(2))
            nv = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", m.group(2)).group(1))
            rows[m.group(1)].update(waves=max(1, min(8, 512 // ((nv + 7) // 8 * 8))), arch_vgpr=int(acc.group(1)) if acc else nv)
    return rows


if __name__ == "__main__":
    print(f"{'kernel':44s} {'instr':>6s} {'mfma':>5s} {'salu':>5s} {'lanes':>5s} {'s_mul':>5s} {'dma':>4s} {'spill':>5s} {'vgpr':>4s} {'scr':>4s} {'w/simd':>6s}")
    srcs = ("conv7.hip", "bwd6.hip")
    with tempfile.TemporaryDirectory() as d:
        asm = compile_asm(srcs, os.environ.get("ISA_COUNTS_KEEP") or d)     # (ISA_COUNTS_KEEP=dir keeps the .s files)
    for src in srcs:
        rows = counts(asm[src])
        names = demangle(list(rows))
        for k, r in rows.items():
            nm = names[k].split("(")[0].replace("(anonymous namespace)::", "").replace("void ", "")
            if "--all" in sys.argv or nm.startswith(("conv7_kernel", "bwd7_kernel")):
                print(f"{nm:44s} {r['instr']:6d} {r['mfma']:5d} {r['salu']:5d} {r['lanes']:5d} {r['smul']:5d} {r['dma']:4d} {r.get('spill', -1):5d} "
                      f"{r.get('vgpr', -1):4d} {r.get('scratch', -1):4d} {r.get('waves', -1):6d}", flush=True)
