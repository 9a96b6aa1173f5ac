"""make_openke_format.py -- store the data files tests/test_openke_format.py reads, so that the
test needs nothing outside the repository.

Runs only where the reference checkout exists (python tests/golden/make_openke_format.py
<reference root>). It copies DATA files the reference ships, byte for byte, xz-compressed, into
tests/golden/openke_format/: the FB15K237 benchmark's train / valid / test triples (the inputs
of n-n.py) with the files n-n.py made from them (the expected outputs), and the FB15K-237-ZS
id maps and test tasks. A file whose compressed size would pass the 1 MiB limit for committed
files is cut at line ends into parts (<name>.0.xz, <name>.1.xz, ...), which the test joins.
"""
import lzma
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "openke_format")
PART = 900 * 1024   # compressed bytes per part, below the 1 MiB limit

FILES = {
    "FB15K237": ("OpenKE/benchmarks/FB15K237",
                 ("train2id.txt", "valid2id.txt", "test2id.txt", "1-1.txt", "1-n.txt", "n-1.txt", "n-n.txt",
                  "test2id_all.txt", "type_constrain.txt")),
    "FB15K-237-ZS": ("origin_data/FB15K-237-ZS",
                     ("entity2ids_zsl.json", "relation2ids.json", "test_tasks_zsl.json")),
}


def pack(src, dst_dir, name):
    with open(src, "rb") as f:
        lines = f.read().splitlines(keepends=True)
    n_parts = 1
    while True:
        step = -(-len(lines) // n_parts)
        parts = [lzma.compress(b"".join(lines[i:i + step]), preset=9 | lzma.PRESET_EXTREME)
                 for i in range(0, len(lines), step)]
        if max(map(len, parts)) <= PART:
            break
        n_parts += 1
    for i, p in enumerate(parts):
        with open(os.path.join(dst_dir, f"{name}.{i}.xz"), "wb") as f:
            f.write(p)
    return [len(p) for p in parts]


def main(ref):
    for sub, (rel, names) in FILES.items():
        d = os.path.join(OUT, sub)
        os.makedirs(d, exist_ok=True)
        for name in names:
            print(sub, name, pack(os.path.join(ref, rel, name), d, name))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit("usage: make_openke_format.py <reference root>")
    main(sys.argv[1])
