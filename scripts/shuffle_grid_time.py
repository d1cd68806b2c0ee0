"""bear_shuffle_rows over whole columns, for the comparison of two builds of the library: the shuffle kernels stride over their range
with a grid of at most SHF_MAX_BLOCKS = 4096 blocks (kernels_shuffle.h), where they launched up to 2^20 blocks before the range
form came.  Times `kernels.shuffle_rows` on 4e7 rows of 20 B and of 13 B, 8e6 rows of 84 B and 1e8 rows of 20 B (HIP events after
settling launches, best of five windows of four launches) and prints one JSON line per shape, labelled by the first argument.

The variant with the former cap is the same sources with one constant changed, built into a library of its own and chosen by
BEAR_AMD_LIB (bear_amd/_lib.py):
    mkdir -p build_variants/src/bear_amd && cp -r include build_variants/src/ && cp -r bear_amd/csrc build_variants/src/bear_amd/
    sed -i 's/#define SHF_MAX_BLOCKS 4096u/#define SHF_MAX_BLOCKS (1u << 20)/' build_variants/src/bear_amd/csrc/kernels_shuffle.h
    make -j16 -C build_variants/src/bear_amd/csrc ../libbear_hip.so          # -> build_variants/src/bear_amd/libbear_hip.so
Then, in one session, the two builds in turn (profiles/shuffle_grid_cap.jsonl is built, variant, built):
    python scripts/shuffle_grid_time.py "grid capped at 4096 blocks" >> profiles/shuffle_grid_cap.jsonl
    BEAR_AMD_LIB=$PWD/build_variants/src/bear_amd/libbear_hip.so python scripts/shuffle_grid_time.py "grid capped at 2^20 blocks (parent)" \\
        >> profiles/shuffle_grid_cap.jsonl
    python scripts/shuffle_grid_time.py "grid capped at 4096 blocks" >> profiles/shuffle_grid_cap.jsonl"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from prot_time import settle

SHAPES = ((40_000_000, (5,), torch.int32), (40_000_000, (13,), torch.uint8), (8_000_000, (21,), torch.int32), (100_000_000, (5,), torch.int32))


def main():
    from bear_amd import kernels
    label = sys.argv[1] if len(sys.argv) > 1 else "library as built"
    dev = torch.device("cuda", 0)
    for n, shape, dtype in SHAPES:
        src = torch.randint(0, 100, (n,) + shape, device=dev).to(dtype).contiguous()
        fn = lambda: kernels.shuffle_rows(src, 1)       # noqa: E731
        settle(fn, cap_s=1.5)
        best = float("inf")
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(4):
                fn()
            e1.record()
            torch.cuda.synchronize()
            best = min(best, e0.elapsed_time(e1) / 4)
        print(json.dumps({"lib": label, "rows": n, "row_bytes": src[0].numel() * src.element_size(), "ms": round(best, 3)}), flush=True)
        del src


if __name__ == "__main__":
    main()
