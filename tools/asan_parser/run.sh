#!/bin/bash
# AddressSanitizer + UBSan, then ThreadSanitizer, over the FASTA/FASTQ front end (host code, no GPU needed): a fuzz corpus of
# mutated files, gzip copies of some and BGZF images, through the block-parallel and the sequential scanner, whose outputs must
# agree.  Both are stand-alone programs built from main.cpp and the parser's sources.  Usage: bash tools/asan_parser/run.sh
set -e
HERE=$(cd "$(dirname "$0")" && pwd); ROOT=$(cd "$HERE/../.." && pwd); W=${TMPDIR:-/tmp}/rk_asan_parser; mkdir -p $W
C=$ROOT/rkmh_amd/csrc; SRCS="$C/rk_pool.cpp $C/rk_parse.cpp $C/rk_parse_blocks.cpp $C/rk_bgzf.cpp"
g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -I$ROOT/include $HERE/main.cpp $SRCS -o $W/parse_asan -lz -lpthread -ldl
g++ -O1 -g -std=c++17 -fsanitize=thread -fno-omit-frame-pointer -I$ROOT/include $HERE/main.cpp $SRCS -o $W/parse_tsan -lz -lpthread -ldl
python3 $HERE/gen.py ${1:-1} $W/corpus ${2:-300}
# (threads, block KB, RKMH_GZ_BLOCKS: 2 = the inflater thread and the pipe-block branch on the gzip copies, small as they are)
for cfg in "4 4 1" "8 16 2" "1 64 1"; do set -- $cfg
  RKMH_PARSE_THREADS=$1 RKMH_PARSE_BLOCK_KB=$2 RKMH_GZ_BLOCKS=$3 $W/parse_asan $W/corpus/*.txt > $W/out_$1.txt 2> $W/err_$1.txt
  echo "threads=$1 block_kb=$2 gz_blocks=$3: sanitizer output $(wc -c < $W/err_$1.txt) bytes"
done
RKMH_PARSE_THREADS=8 RKMH_PARSE_BLOCK_KB=16 RKMH_GZ_BLOCKS=2 $W/parse_tsan $W/corpus/*.txt > $W/out_tsan.txt 2> $W/err_tsan.txt || true
echo "ThreadSanitizer, threads=8 block_kb=16 gz_blocks=2: $(grep -c 'WARNING: ThreadSanitizer' $W/err_tsan.txt || true) reports, $(wc -c < $W/err_tsan.txt) bytes of output"
test ! -s $W/err_tsan.txt
# a gzip copy gives what its plain file gives
for z in $W/corpus/*.gz.txt; do
  test "$(grep -F "${z%.gz.txt}.txt " $W/out_8.txt | cut -d' ' -f2-)" = "$(grep -F "$z " $W/out_8.txt | cut -d' ' -f2-)" || { echo "gzip copy differs: $z"; exit 1; }
done
cmp $W/out_4.txt $W/out_1.txt && cmp $W/out_8.txt $W/out_1.txt && cmp $W/out_tsan.txt $W/out_1.txt && echo "parallel == sequential on the whole corpus"
