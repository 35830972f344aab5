"""Condense the `-s` output of tests/test_gpu_glue_f64.py into the table kept as profiles/glue_f64_errors.txt:

    python -m pytest tests/test_gpu_glue_f64.py -m gpu -q -s > log.txt;  python dev/glue_f64_table.py log.txt > profiles/glue_f64_errors.txt

One line per (entry point, type, head geometry, kind of case) over all its positions, batch sizes, split counts and passes: the
number of cases, the largest per-(row, head) error e of the kernel and of the 16-bit torch formulation in units of u, and the
largest e / allowance of a case (the test asserts <= 1)."""
import collections
import re
import sys

ATTN = re.compile(r"GLUE_F64 (\S+?)(?:/\d+ pass \d)? (bf16|fp16) heads=(\S+) bs=\d+ T=(\d+) p0=\d+ S=\d+ (\w+): e ([\d.]+) u, allowed ([\d.]+) u \(torch16 ([\d.]+) u\)")
ELEM = re.compile(r"GLUE_F64 (add_rmsnorm|swiglu) (bf16|fp16) (?:rows=\d+ dim=(\d+) (\w+)|bs=\d+ il=(\d+)).*largest error / bound ([\d.]+)")


def main(path):
    attn = collections.defaultdict(lambda: [0, 0.0, 0.0, 0.0])
    elem = collections.defaultdict(lambda: [0, 0.0])
    rope, tail = [], ""
    for line in open(path):
        line = line.lstrip(".FEsx").rstrip()
        m = ATTN.match(line)
        if m:
            entry, dt, heads, T, kind, e, allow, t16 = m.groups()
            if entry == "prefill_attn" and int(T) >= 2048:
                heads += " T=2048"
            a = attn[(entry, dt, heads, kind)]
            a[0] += 1
            a[1], a[2], a[3] = max(a[1], float(e)), max(a[2], float(t16)), max(a[3], float(e) / float(allow))
            continue
        m = ELEM.match(line)
        if m:
            op, dt, dim, kind, il, rel = m.groups()
            a = elem[(op, dt, f"dim={dim} {kind}" if dim else f"il={il}")]
            a[0] += 1
            a[1] = max(a[1], float(rel))
            continue
        if line.startswith("GLUE_ROPE") and " total:" in line:
            rope.append(line)
        if " passed" in line or " failed" in line:
            tail = line
    print("tests/test_gpu_glue_f64.py on one MI355X: errors against the float64 references (tests/glue_ref.py); u = 2^-8 (bf16), 2^-11 (fp16)")
    print(f"pytest: {tail}\n")
    print("Attention: e = max_d |got - ref64| / max_d |ref64| per (row, head); allowance per case = 2 max(e of the 16-bit torch formulation, 2u)")
    print(f"{'entry point':18s} {'type':5s} {'heads (hl/kvl x d)':22s} {'kind':7s} {'cases':>6s} {'max e / u':>10s} {'torch16 / u':>12s} {'max e / allowed':>16s}")
    for (entry, dt, heads, kind), (n, e, t16, rel) in sorted(attn.items()):
        print(f"{entry:18s} {dt:5s} {heads:22s} {kind:7s} {n:6d} {e:10.2f} {t16:12.2f} {rel:16.2f}")
    print("\nRMSNorm / SwiGLU: largest |got - ref64| / ((2u + u^2 + 1e-5) |ref64| + smallest normal) (asserted <= 1)")
    for (op, dt, what), (n, rel) in sorted(elem.items()):
        print(f"{op:12s} {dt:5s} {what:28s} {n:4d} cases  {rel:6.3f}")
    print("\nRope bits (lookup rows are compared bit for bit and do not appear above)")
    for line in rope:
        print(line)


if __name__ == "__main__":
    main(sys.argv[1])
