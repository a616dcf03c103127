"""dev tool: cut a tools/step_order.py listing to the serial `post` stage (usage: post_order.py STEP_ORDER.txt [tail]): the launches on the
queue of the attention kernels from the first one behind the expert banks' forward (the sigmoid of the swap weights, or failing that the
first attention forward) to the two launches behind that sigmoid's backward (failing that, `tail` = 25 launches behind the last
attention backward), with their count and summed duration."""
import re
import sys

lines = [l.rstrip("\n") for l in open(sys.argv[1])]
tail = int(sys.argv[2]) if len(sys.argv) > 2 else 25


def q(l):
    return re.search(r"q\s*(\d+)", l).group(1)


def us(l):
    return float(re.search(r"q\s*\d+\s+([\d.]+) us", l).group(1))


qa = q([l for l in lines if "attn_bwd_merged" in l][-1])       # the fusion stage's attention backward: the last one of the step
mine = [i for i, l in enumerate(lines) if q(l) == qa]
bwd = [i for i in mine if "attn_bwd_merged" in lines[i]][-2:]
fwd = [i for i in mine if "attn_fwd" in lines[i] and i < bwd[0]][-2:]
sig = [i for i in mine if i < fwd[0] and "sigmoid" in lines[i]]
start = sig[-1] if sig else fwd[0]
after = [i for i in mine if i > bwd[-1]]
sb = [k for k, i in enumerate(after) if "sigmoid_bwd" in lines[i]]
after = after[:sb[0] + 3] if sb else after[:tail]
end = after[-1] if after else bwd[-1]
sel = [i for i in mine if start <= i <= end]
attn = sum(us(lines[i]) for i in sel if "attn_" in lines[i])
tot = sum(us(lines[i]) for i in sel)
print(f"--- post on queue {qa}: {len(sel)} launches, {tot:.1f} us summed kernel time, {attn:.1f} us of it in {sum('attn_' in lines[i] for i in sel)} attention launches, "
      f"{tot - attn:.1f} us in the other {len(sel) - sum('attn_' in lines[i] for i in sel)}; wall {float(lines[end].split()[0]) + us(lines[end]) - float(lines[start].split()[0]):.1f} us")
for i in sel:
    print(lines[i])
