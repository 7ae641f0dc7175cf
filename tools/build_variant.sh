#!/bin/bash
# tools/build_variant.sh NAME [-DFLAG ...]: sources of csrc/ (SRC="gemm gemm_generic" by default: the GEMM sources;
# gemm compiles the choice, the trace and, from gemm_v4.hpp and gemm_tiled.hpp, gemm_kernel_v4, v7 and v8; gemm_generic compiles gemm_kernel) rebuilt with extra defines into
# tools/variants/libpvnative_NAME.so (the other objects come from the regular in-tree build); select it with
# PV_NATIVE_LIB=tools/variants/libpvnative_NAME.so
# Switches of the ViT forward's kernels: -DPV_STORE_CONSUMED=P -DPV_STORE_TAP=P (store policy of the large outputs, P = 0 plain,
# 1 nt, 2 sc1, 3 sc1 nt; pv_common.hpp: SRC="gemm gemm_generic rowops attention"), -DPV_ATTN_V_ROWS=0, -DPV_ATTN_VROWS_WAVES=3 (SRC=attention), -DPV_GEMM_MFMA=32 (the bf16 GEMMs v4 / v7 / v8 on v_mfma_f32_32x32x16_bf16 instead of 16x16x32; SRC=gemm is enough)
# Switches of the filtered SAE encoder: -DPV_SEL_TRACE, -DPV_SEL_WAVES=N (SRC=sae_enc: the top-k select kernel's time stamps / launch bound), -DPV_ENC_TRACE (SRC="sae_enc sae_enc_gemm": the filter GEMM's time stamps), -DPV_DEC_ROWS=N (SRC=sae)
# -DPV_GEMM_RESID_PARK=0 (gemm_kernel_v7's full-line residual instances without the residual park: the residual rows loaded inside the store epilogue; SRC=gemm is enough)
set -e
cd "$(dirname "$0")/.."
name=$1; shift
src=${SRC:-gemm gemm_generic}
mkdir -p tools/variants
python -m vit_prisma_amd.build >/dev/null
# (SRC may list several sources: SRC="gemm rowops attention")
objs=$(ls vit_prisma_amd/csrc/_obj/*.o)
vobjs=""
for one in $src; do
  hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wno-unused-function -ffp-contract=off -Iinclude "$@" -c vit_prisma_amd/csrc/$one.hip -o tools/variants/${one}_$name.o
  objs=$(echo "$objs" | grep -v "/$one.o")
  vobjs="$vobjs tools/variants/${one}_$name.o"
done
hipcc -shared -fPIC --offload-arch=gfx950 -o tools/variants/libpvnative_$name.so $objs $vobjs
rm $vobjs
echo built tools/variants/libpvnative_$name.so
