# development aid: the vector and LDS counters of sd_sift (and of every other kernel of the step), one stage after the other (tools/perf_probe.py all)
# (rocprofv3 --pmc, no other tracing).  PMC="..." bash tools/pmc_sift.sh: other counters (one pass holds about eight);
# CORNETTO_LIB=... : another build of the library (A/B of kernel variants on one box).  The table goes to stdout, everything else to a temporary folder.
R=$PWD
D=$(mktemp -d)
cd $D && export TMPDIR=$D
timeout 600 rocprofv3 --pmc ${PMC:-SQ_INSTS_VALU SQ_INSTS_LDS SQ_LDS_IDX_ACTIVE SQ_LDS_BANK_CONFLICT SQ_WAVES} -d $D/pmc --output-format csv -- python3 $R/tools/perf_probe.py all --mbases 3160 --reps 1 --simple-cov 1 > $D/run.log 2>&1 || { tail -5 $D/run.log; exit 1; }
python3 - $D/pmc <<'PY'
import csv,glob,collections,re,sys
agg=collections.defaultdict(lambda: collections.defaultdict(float)); n=collections.defaultdict(set)
for f in glob.glob(sys.argv[1]+"/**/*_counter_collection.csv",recursive=True):
    for r in csv.DictReader(open(f)):
        k=re.split(r"[<(]", r["Kernel_Name"].replace("void ","").replace("(anonymous namespace)::",""))[0][-40:]
        agg[k][r["Counter_Name"]]+=float(r["Counter_Value"]); n[k].add(r["Dispatch_Id"])
rows=[]
for k,c in agg.items():
    d=max(1,len(n[k]))
    tot=sum(v for kk,v in c.items() if kk.startswith("SQ_INSTS"))
    rows.append((tot/d, k, d, {kk.replace("SQ_INSTS_","").replace("SQ_",""): round(v/d/1e6,2) for kk,v in c.items()}))
for t,k,d,c in sorted(rows,reverse=True)[:16]: print("%9.1f M wave-instr/launch  %-40s x%d %s"%(t/1e6,k,d,c))
PY
cd $R
rm -rf $D
