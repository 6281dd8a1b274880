"""Cost of the bottom regions of the full GP's factorisation from a rocprofv3 kernel trace of the
unit (tools/trace_unit.py): per persistent launch of the LAST unit, the time from its start to
the start of the first 128-tile GEMM launch after it — for two 20-tile blocks that is the blocks
plus the 2560-level W, SYRK ‖ T and L⁻¹21 launches between and behind them.

  python tools/dag_region.py <trace dir>/run_kernel_trace.csv [persistent launches per unit = 8]
"""
import csv
import sys


def main():
    rows = sorted(csv.DictReader(open(sys.argv[1])), key=lambda r: int(r["Start_Timestamp"]))
    per_unit = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    dag = [i for i, r in enumerate(rows) if "potrf_dag_kernel" in r["Kernel_Name"]][-per_unit:]
    group = per_unit // 4            # persistent launches per 5120 region
    tot = 0.0
    for a in range(0, per_unit, group):
        i0, i1 = dag[a], dag[a + group - 1]
        s = int(rows[i0]["Start_Timestamp"])
        nxt = next(r for r in rows[i1 + 1:] if "gemm_f64_kernel" in r["Kernel_Name"] and ", 128>" in r["Kernel_Name"])
        ms = (int(nxt["Start_Timestamp"]) - s) / 1e6
        blocks = " ".join("%.3f" % ((int(rows[i]["End_Timestamp"]) - int(rows[i]["Start_Timestamp"])) / 1e6)
                          for i in dag[a:a + group])
        print("region %d: %.3f ms (persistent launches: %s ms)" % (a // group, ms, blocks))
        tot += ms
    print("four regions: %.3f ms" % tot)


if __name__ == "__main__":
    main()
