"""Compare two device assembly listings (hipcc --cuda-device-only -S with the
Makefile's flags; parent, new) kernel by kernel under their mangled names:
the text of each kernel up to its .Lfunc_end, comments and blank lines
dropped, local label numbers normalised.  For csrc/dna.hip, whose kernels sit
in an anonymous namespace (profiles/r11/generic_refactor/compare_asm.py keys
kernels by their demangled name cut at the first parenthesis, which is
"(anonymous namespace)" for all of them).

    python compare_asm_by_name.py parent_dna.s new_dna.s
"""
import re
import sys


def funcs(path):
    d, cur = {}, None
    for line in open(path):
        m = re.match(r'^(_Z\S+):\s*(;.*)?$', line)
        if m:
            cur = m.group(1)
            d[cur] = []
            continue
        if cur is None:
            continue
        if line.startswith('.Lfunc_end'):
            cur = None
            continue
        t = line.strip()
        if not t or t.startswith(';'):
            continue
        line = re.sub(r'Header=BB\d+_', 'Header=BBN_',
                      re.sub(r'\.L(BB|JTI|tmp|func_begin|func_end|CPI)\d+_?', r'.L\1N_', line))
        d[cur].append(re.sub(r';.*', '', line).rstrip())
    return d


a, b = funcs(sys.argv[1]), funcs(sys.argv[2])
only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
diff = [k for k in sorted(set(a) & set(b)) if a[k] != b[k]]
print(f"kernels: parent {len(a)}, new {len(b)}; only in parent {len(only_a)}, only in new {len(only_b)}, "
      f"identical {len(set(a) & set(b)) - len(diff)}, different {len(diff)}")
for k in only_a + only_b + diff:
    print("  ", k)
sys.exit(1 if only_a or only_b or diff else 0)
