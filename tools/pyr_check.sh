#!/bin/bash
# Pyramid check after a kernel change: the extraction tests, one benchmark step with the pyramid
# stamps (ORBGPU_PYR_STAMPS) and one benchmark line.  Outputs under $O (default out/pyr_check).
# A step that fails ends the script.
O=${O:-out/pyr_check}
mkdir -p $O
EX="--full --no-cpu-baseline --no-ba --no-stereo --no-pose --no-bow --no-single --no-c4 --no-matchers"
timeout -k 10 200 python -u -m pytest tests/test_extract_gpu.py -x -q --timeout 120 --timeout-method thread > $O/t_ext.log 2>&1 || { tail -3 $O/t_ext.log; exit 1; }
tail -3 $O/t_ext.log
ORBGPU_PYR_STAMPS=1 timeout -k 10 100 python3 bench.py --steps 1 --warmup 1 $EX > $O/st.json 2> $O/st.err || { tail -5 $O/st.err; exit 1; }
grep pyr-stamps $O/st.err | tail -8
timeout -k 10 100 python3 bench.py $EX > $O/b1.json 2>$O/b1.err || { tail -5 $O/b1.err; exit 1; }
cat $O/b1.json
