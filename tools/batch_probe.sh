# configs[1] throughput vs frames per step (bench.py --batch), one box
set -e
cd "$(dirname "$0")/.."; O=out/bp; mkdir -p $O
for b in ${@:-64 128 64}; do
  timeout -k 10 300 python3 bench.py --full --no-cpu --seq-frames 0 --large-batch 0 --runs 3 --batch $b > $O/b$b.json 2> $O/b$b.err
  python3 -c "import json;d=json.load(open('$O/b$b.json'));print($b, round(d['value'],1), round(d['ms_per_step'],3), d['timed_runs'])"
done
