"""The tables of profiles/r05_row_families_parity.md from the report tests/test_gpu_row_families.py writes:
    python tools/row_families_table.py <path to row_families_parity.json>"""
import json
import sys

d = json.load(open(sys.argv[1]))
fams = d["families"]
short = {"control":"ctrl","noise_only":"noise","noise_free":"nfree","constant":"const","saturated":"sat","full_scale":"full","negative":"neg","pileup":"pile","tail":"tail","early":"early","late":"late","tau_short":"tau/2","tau_long":"2tau","slow_rise":"slow","tiny":"tiny"}
out = []
out.append("| route | " + " | ".join(short[f] for f in fams) + " |")
out.append("|---|" + "---|" * len(fams))
details = []
for route in sorted(d["routes"]):
    r = d["routes"][route]
    cells = []
    for f in fams:
        worst, worst_name, diff = 0.0, None, 0
        for name, v in r.get(f, {}).items():
            if "worst_over_bar" in v and v["worst_over_bar"] >= worst:
                worst, worst_name = v["worst_over_bar"], name
            if "rows_differing" in v and "reported" not in name and "binds" not in name and "counted" not in name:
                diff += v["rows_differing"]
        cells.append((f"{worst:.2f}" if worst_name else "-") + (f" / **{diff}**" if diff else " / 0"))
    out.append(f"| {route} | " + " | ".join(cells) + " |")
print("\n".join(out))
print()
# reported (not asserted) index differences and second-term binds
for route in sorted(d["routes"]):
    r = d["routes"][route]
    rep = {}
    for f in fams:
        for name, v in r.get(f, {}).items():
            if ("reported" in name or "binds" in name or "counted" in name) and v.get("rows_differing"):
                rep.setdefault(name, {})[short[f]] = f'{v["rows_differing"]}/{v["of"]}'
    for name, m in sorted(rep.items()):
        print(f"- {route}: {name}: " + ", ".join(f"{k} {v}" for k, v in m.items()))
print()
# outputs above 0.7 of the bar
for route in sorted(d["routes"]):
    r = d["routes"][route]
    for f in fams:
        for name, v in r.get(f, {}).items():
            if v.get("worst_over_bar", 0) > 0.7:
                print(f"- {route}: {name}: {short[f]} {v['worst_over_bar']:.2f}")
