"""Convert an IAM-layout word folder to the bucketed reading format main.py trains on (the reference runs this from main.py:62-63
when read_dir is missing):

    python -m scrabble_gan_amd.prepare_data --gin configs/scrabble_gan_mi355x.gin [--raw-dir DIR] [--read-dir DIR]

io.raw_dir, io.read_dir, io.input_dim and io.bucket_size come from the gin file; each has an override flag."""
from __future__ import annotations

import argparse
import os


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--gin", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "configs",
                                                  "scrabble_gan_mi355x.gin"))
    ap.add_argument("--raw-dir", default=None, help="folder with the word PNGs (default: io.base_path + io.raw_dir)")
    ap.add_argument("--read-dir", default=None, help="output folder of the buckets (default: io.base_path + io.read_dir)")
    ap.add_argument("--transcriptions", default=None, help="words.txt (default: <raw-dir>/../gt/words.txt)")
    ap.add_argument("--height", type=int, default=None, help="image height (default: io.input_dim[0]); a character is height/2 wide")
    ap.add_argument("--bucket-size", type=int, default=None, help="longest word kept (default: io.bucket_size)")
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    from . import gin_config as gin
    from .main import setup_io
    gin.parse_config_file(args.gin)
    in_dim, _, _, _, bucket_size, _, _, _, raw_dir, read_dir, _ = setup_io()
    if args.height:
        in_dim = (args.height,) + tuple(in_dim[1:])
    from .dinterface import convert_to_gan_reading_format_save
    convert_to_gan_reading_format_save(args.raw_dir or raw_dir, args.read_dir or read_dir, in_dim, args.bucket_size or bucket_size,
                                       transcriptions=args.transcriptions)


if __name__ == "__main__":
    main()
