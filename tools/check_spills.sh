#!/bin/bash
# Reports every kernel of the fast aggregate instantiations and of the string functions (with and without arguments), of string matching, of the conditional functions and of the casts that spills VGPRs (scratch traffic in a streaming kernel is a 2x cliff)
# or uses scratch memory without spilling (a by-value kernel argument indexed at run time lands there: 3.7x slower, found once).
cd "$(dirname "$0")/../naive_query_engine_amd/csrc"
for pv in 0:0 0:1 1:0 1:1 2:0 2:1 3:0 3:1 4:0; do p=${pv%:*}; v=${pv#*:}
  ( /opt/rocm/bin/hipcc -O3 -std=c++17 --offload-arch=gfx950 -munsafe-fp-atomics -fno-gpu-rdc $EXTRA -DNQE_FAST_PRED=$p -DNQE_FAST_VNULL=$v -c aggregate_fast_inst.hip -o /dev/null -Rpass-analysis=kernel-resource-usage 2>&1 \
    | grep -E "Function Name|VGPRs:|ScratchSize|VGPRs Spill" | sed 's/.*remark: *//; s/ \[-Rpass.*//' | paste - - - - | awk '$NF != 0 || $(NF-3) != 0' | sed 's/Function Name: _ZN3nqe3agg12_GLOBAL__N_1//' > /tmp/spills_${p}_${v}.txt ) &
done
# ... and of the string functions' kernels (string_fn.hip: str_case, str_reverse, str_length, str_trim_bounds, str_trim_copy)
( /opt/rocm/bin/hipcc -O3 -std=c++17 --offload-arch=gfx950 -munsafe-fp-atomics -fno-gpu-rdc $EXTRA -c string_fn.hip -o /dev/null -Rpass-analysis=kernel-resource-usage 2>&1 \
    | grep -E "Function Name|VGPRs:|ScratchSize|VGPRs Spill" | sed 's/.*remark: *//; s/ \[-Rpass.*//' | paste - - - - | awk '$NF != 0 || $(NF-3) != 0' | sed 's/Function Name: _ZN3nqe12_GLOBAL__N_1//' > /tmp/spills_string_fn.txt ) &
# ... and of the string functions with arguments (string_args.hip: str_substr_bounds, str_repeat_lengths, str_repeat_copy, str_replace_same, str_replace_count, str_replace_emit, str_args_validity)
( /opt/rocm/bin/hipcc -O3 -std=c++17 --offload-arch=gfx950 -munsafe-fp-atomics -fno-gpu-rdc $EXTRA -c string_args.hip -o /dev/null -Rpass-analysis=kernel-resource-usage 2>&1 \
    | grep -E "Function Name|VGPRs:|ScratchSize|VGPRs Spill" | sed 's/.*remark: *//; s/ \[-Rpass.*//' | paste - - - - | awk '$NF != 0 || $(NF-3) != 0' | sed 's/Function Name: _ZN3nqe12_GLOBAL__N_1//' > /tmp/spills_string_args.txt ) &
# ... and of string matching (string_match.hip: str_match_anchor, str_match_scan)
( /opt/rocm/bin/hipcc -O3 -std=c++17 --offload-arch=gfx950 -munsafe-fp-atomics -fno-gpu-rdc $EXTRA -c string_match.hip -o /dev/null -Rpass-analysis=kernel-resource-usage 2>&1 \
    | grep -E "Function Name|VGPRs:|ScratchSize|VGPRs Spill" | sed 's/.*remark: *//; s/ \[-Rpass.*//' | paste - - - - | awk '$NF != 0 || $(NF-3) != 0' | sed 's/Function Name: _ZN3nqe12_GLOBAL__N_1//' > /tmp/spills_string_match.txt ) &
# ... and of the conditional functions (conditional.hip: cond_words, cond_bits, cond_str_lengths, cond_str_copy)
( /opt/rocm/bin/hipcc -O3 -std=c++17 --offload-arch=gfx950 -munsafe-fp-atomics -fno-gpu-rdc $EXTRA -c conditional.hip -o /dev/null -Rpass-analysis=kernel-resource-usage 2>&1 \
    | grep -E "Function Name|VGPRs:|ScratchSize|VGPRs Spill" | sed 's/.*remark: *//; s/ \[-Rpass.*//' | paste - - - - | awk '$NF != 0 || $(NF-3) != 0' | sed 's/Function Name: _ZN3nqe12_GLOBAL__N_1//' > /tmp/spills_conditional.txt ) &
# ... and of the casts (cast.hip: cast_fixed, cast_parse, cast_text_lengths, cast_text_write)
( /opt/rocm/bin/hipcc -O3 -std=c++17 --offload-arch=gfx950 -munsafe-fp-atomics -fno-gpu-rdc $EXTRA -c cast.hip -o /dev/null -Rpass-analysis=kernel-resource-usage 2>&1 \
    | grep -E "Function Name|VGPRs:|ScratchSize|VGPRs Spill" | sed 's/.*remark: *//; s/ \[-Rpass.*//' | paste - - - - | awk '$NF != 0 || $(NF-3) != 0' | sed 's/Function Name: _ZN3nqe12_GLOBAL__N_1//' > /tmp/spills_cast.txt ) &
wait
cat /tmp/spills_*.txt | cut -c1-200
echo "kernels with VGPR spills or scratch: $(cat /tmp/spills_*.txt | wc -l)"
