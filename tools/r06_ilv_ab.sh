for lib in "" devlibs/lib_ilv.so; do
  for r in 1 2 3; do CONV3P_HIP_LIB=$lib timeout 200 python bench.py --full --no-cpu --no-extra 2>/dev/null | tail -1 | python -c "
import sys, json
d = json.loads(sys.stdin.read()); print('cfg2 lib=$lib', d['ms_per_step'], {k: round(v, 4) for k, v in d['roofline']['kernel_ms_per_step'].items()})"; done
  for r in 1 2; do CONV3P_HIP_LIB=$lib timeout 200 python bench.py --full --no-cpu --no-extra --serial 2>/dev/null | tail -1 | python -c "
import sys, json
d = json.loads(sys.stdin.read()); print('serial lib=$lib', d['ms_per_step'], {k: round(v, 4) for k, v in d['roofline']['kernel_ms_per_step'].items()})"; done
  for r in 1 2; do echo -n "cfg4 lib=$lib: "; CONV3P_HIP_LIB=$lib timeout 200 python tools/cfg4_step.py 2>/dev/null | tail -1; done
done
CONV3P_HIP_LIB=devlibs/lib_ilv.so timeout 1300 python -m pytest tests -m gpu -x -q 2>&1 | tail -5
