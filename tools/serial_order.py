"""dev tool: cut a tools/step_order.py listing to the serial stages (usage: serial_order.py STEP_ORDER.txt): pre (up to the first trunk conv), the launches behind each trunk's pooled read
on its queue (router head), pre_bwd (the trailing run of the first queue)."""
import sys, re
lines = [l.rstrip("\n") for l in open(sys.argv[1])]
def q(l): return re.search(r"q\s*(\d+)", l).group(1)
first = next(i for i, l in enumerate(lines) if "conv6_split_kernel" in l)
out = ["--- pre (launches before the first router-trunk conv)"] + lines[:first]
for i, l in enumerate(lines):
    if "gn1_relu_mean_kernel" in l:
        out.append(f"--- router head on queue {q(l)} (the pooled read and the launches behind it on its queue, up to the routing kernels)")
        k, n = i, 0
        while k < len(lines) and n < 14:
            if q(lines[k]) == q(l):
                out.append(lines[k]); n += 1
            k += 1
q0 = q(lines[0])
j = len(lines)
while j > 0 and q(lines[j - 1]) == q0:
    j -= 1
out += ["--- pre_bwd (the trailing launches of the first queue)"] + lines[j:]
print("\n".join(out))
