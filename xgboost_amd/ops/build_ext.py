"""Build the HIP kernel library for gfx950 (in-tree, travels with the
repo snapshot).  Invoked by __graft_entry__.build() and on demand."""
import glob
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp")
OUT = os.path.join(HERE, "libgbt_hip.so")

SOURCES = ["hist.hip", "partition.hip", "evaluate.hip", "compress.hip",
           "predict.hip", "predict_bins.hip", "predict_csr.hip", "shap.hip",
           "shap_paths.hip", "shap_ix.hip", "shap_csr.hip",
           "driver.hip", "csr.hip", "gpair.hip", "mt_evaluate.hip",
           "cpu_hist.cpp", "lambdarank.hip", "rank_metric.hip",
           "shap_saabas.hip", "lambdarank_slab.hip", "softmax_gpair.hip",
           "mvs_sample.hip", "evaluate_cat.hip"]

# Sources compiled on their own, with flags the other kernels were not
# measured under: the ranking, Saabas and softmax-gradient kernels keep the
# compiler from pairing fp32 operations into packed instructions and print
# the per-kernel resource usage (registers, LDS, scratch, occupancy;
# profiles/lambdarank_mi355x.md, profiles/shap_approx_mi355x.md,
# profiles/multiclass_mi355x.md).
_RANK_FLAGS = ["-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops",
               "-Rpass-analysis=kernel-resource-usage"]
OWN_FLAGS = {
    "lambdarank.hip": _RANK_FLAGS,
    "lambdarank_slab.hip": _RANK_FLAGS,
    "rank_metric.hip": _RANK_FLAGS,
    "shap_saabas.hip": _RANK_FLAGS,
    "softmax_gpair.hip": _RANK_FLAGS,
    # holds the batched quantise kernel that follows softmax_gpair.hip
    "gpair.hip": _RANK_FLAGS,
    # its exact scores also need -ffp-contract=off and the default,
    # correctly rounded sqrtf and division: both hold in `common` below
    "mvs_sample.hip": _RANK_FLAGS,
    # fp64 and int64 only: just the resource report
    # (profiles/categorical_mi355x.md)
    "evaluate_cat.hip": ["-Rpass-analysis=kernel-resource-usage"],
}


def build(force: bool = False) -> str:
    sources = [os.path.join(SRC, s) for s in SOURCES
               if os.path.exists(os.path.join(SRC, s))]
    if not force and os.path.exists(OUT):
        newest = max(os.path.getmtime(s) for s in sources +
                     glob.glob(os.path.join(SRC, "*.h")))
        if os.path.getmtime(OUT) >= newest:
            return OUT
    hipcc = os.environ.get("HIPCC", "hipcc")
    common = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17",
              "-ffp-contract=off",  # bit-match the numpy fp64 oracle
              "-fopenmp",           # native CPU hist/partition (cpu_hist.cpp)
              "-fPIC"]
    with tempfile.TemporaryDirectory() as tmp:
        inputs = []
        for src in sources:
            own = OWN_FLAGS.get(os.path.basename(src))
            if own is None:
                inputs.append(src)
                continue
            obj = os.path.join(tmp, os.path.basename(src) + ".o")
            cmd = common + own + ["-c", src, "-o", obj]
            print("+", " ".join(cmd), flush=True)
            subprocess.check_call(cmd)
            # ahead of the sources: hipcc's "-x hip" in front of a .hip
            # file holds for every file after it, objects included
            inputs.insert(0, obj)
        cmd = common + ["-shared", "-o", OUT] + inputs
        print("+", " ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    return OUT


if __name__ == "__main__":
    build(force="--force" in sys.argv)
