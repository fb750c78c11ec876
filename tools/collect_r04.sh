#!/bin/bash
# tools/collect_r04.sh OUTDIR : what profiles/r04 holds, collected on the GPU box in one go:
#   the default bench line (headline + also_config2/3/5), per BASELINE config the bench line, rocprofv3 --kernel-trace --stats of
#   the same command and FETCH_SIZE / WRITE_SIZE passes (one counter per run); the same three for the NTT-domain product
#   kernel (tools/domain_bench.py); the sustained headline (400 steps) with rocm-smi beside it and the in-kernel clock of a
#   stamp build; sweeps; RNS pipeline rows.
out=$1; mkdir -p $out
cd /tmp && export TMPDIR=/tmp; cd $GRAFT_REPO_ROOT
timeout 900 python3 bench.py --full > $out/bench_default.json 2> $out/bench_default.err
for c in 4 2 3 5; do
  st="--steps 20 --warmup 3"; [ $c = 5 ] && st="--steps 10 --warmup 2"
  timeout 900 python3 bench.py --full --config $c $st --no-also > $out/bench_config$c.json 2> $out/bench_config$c.err
  timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d $out/kt$c -- python3 bench.py --full --config $c $st --no-cpu-baseline --headline-only > $out/bench_config${c}_under_rocprofv3.json 2> $out/kt$c.log
  for ctr in FETCH_SIZE WRITE_SIZE; do
    timeout 900 rocprofv3 --kernel-trace --pmc $ctr --output-format csv -d $out/pmc$c/$ctr -- python3 bench.py --full --config $c --steps 3 --warmup 1 --no-cpu-baseline --headline-only > $out/pmc${c}_$ctr.log 2>&1
  done
done
python3 tools/pmc_kernels.py $out > $out/pmc_per_kernel.txt 2>&1
# the NTT-domain product kernels: kernel trace + traffic counters over tools/domain_bench.py (2^14: one launch; 2^16: block launch + column pass)
dargs="--logn 14 16 --k 1 3 --steps 4"
timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d $out/kt_dot -- python3 tools/domain_bench.py $dargs > $out/domain_bench_under_rocprofv3.txt 2> $out/kt_dot.log
for ctr in FETCH_SIZE WRITE_SIZE; do
  timeout 600 rocprofv3 --kernel-trace --pmc $ctr --output-format csv -d $out/pmc_dot/$ctr -- python3 tools/domain_bench.py $dargs > $out/pmc_dot_$ctr.log 2>&1
done
python3 tools/pmc_dot.py $out > $out/pmc_dot_per_kernel.txt 2>&1
timeout 900 python3 tools/domain_bench.py --logn 8 10 12 13 14 15 16 17 --k 1 2 3 8 > $out/domain_bench.txt 2>&1
timeout 600 python3 tools/domain_bench.py --logn 12 14 16 --k 1 3 --bits 51 52 60 --no-broadcast > $out/domain_bench_moduli.txt 2>&1
# sustained headline: 400 back-to-back steps (about 3 s), rocm-smi power / clocks beside it; in-kernel clock from the stamp build
bash tools/exp_smi.sh $out/sustained python3 bench.py --full --steps 400 --warmup 5 --no-cpu-baseline --headline-only
mv $out/sustained.log $out/bench_config4_sustained.json; mv $out/sustained.smi $out/rocm_smi_power_clock_during_sustained_bench.txt
if [ -f build/libntt_stamps.so ]; then NTT_LIB=build/libntt_stamps.so timeout 300 python3 tools/stamps.py > $out/phase_stamps_and_clock.txt 2>&1; fi
timeout 600 python3 tools/sweep.py --logn 8 9 10 11 12 13 14 15 16 17 --ops fwd inv --qs 0x80000001c0001 --bytes 16e9 > $out/sweep_sizes.txt 2>&1
timeout 600 python3 tools/sweep.py --logn 12 14 16 --ops fwd inv mul --arith auto u64 --qs 0xffffffff00001 --bytes 8e9 > $out/sweep_52bit_modulus.txt 2>&1
timeout 600 python3 tools/sweep.py --logn 8 9 10 11 12 13 14 15 16 17 --ops mul --qs 0x80000001c0001 --bytes 8e9 > $out/sweep_products.txt 2>&1
# moduli of 2^52 and more (wide integer policy): 57- and 60-bit primes that serve every size up to 2^17
timeout 600 python3 tools/sweep.py --logn 10 12 13 14 15 16 17 --ops fwd inv mul --qs 0x1fffffffffc0001 0xffffffffffc0001 --bytes 4e9 > $out/sweep_integer_moduli.txt 2>&1
(for loop in 1 0; do NTT_RNS_LOOP=$loop timeout 300 python3 tools/pipeline_bench.py; NTT_RNS_LOOP=$loop timeout 300 python3 tools/pipeline_bench.py --logn 16 --batch 1024; NTT_RNS_LOOP=$loop timeout 300 python3 tools/pipeline_bench.py --logn 15 --batch 2048; done; timeout 300 python3 tools/pipeline_bench.py --logn 14 --batch 4096) > $out/pipeline_rns.txt 2>&1
(for lg in 14 16; do for limbs in 4 16; do for b in 1 2 8 64; do
  for loop in 1 0; do NTT_RNS_LOOP=$loop timeout 120 python3 tools/pipeline_bench.py --logn $lg --limbs $limbs --batch $b --steps 10; done
done; done; done) > $out/pipeline_rns_small_batch.txt 2>&1
if [ -x oracle/_ref/ntt-variants-bench-dropin ]; then timeout 600 oracle/_ref/ntt-variants-bench-dropin > $out/reference_bench_driver_dropin.txt 2>&1; fi
rm -rf $out/kt*/*/*agent_info.csv
tail -1 $out/bench_default.json | cut -c1-300; cat $out/pmc_per_kernel.txt $out/pmc_dot_per_kernel.txt
