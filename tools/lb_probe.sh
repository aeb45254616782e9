set -e
cd "$(dirname "$0")/.."; O=out/lb; mkdir -p $O
for b in ${@:-32 64}; do
  timeout -k 10 300 python3 bench.py --full --no-cpu --seq-frames 0 --runs 1 --steps 6 --large-batch $b > $O/b$b.json 2> $O/b$b.err
  python3 -c "import json;d=json.load(open('$O/b$b.json'));l=d['large'];print($b, round(l['value'],1), l['kernel_ms_per_step'])"
done
