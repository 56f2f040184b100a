"""Re-blocks a tensor file as BGZF: `python -m clairvoyante_amd.bgzf IN OUT [--level N]`.

IN is read the way callVar reads it (plain text, any gzip, BGZF; `PIPE` for standard input); OUT holds the same text as
independent gzip members of 65 280 input bytes (utils_v2.BgzfWriter), which `gzip -dc` and every gzip reader take as
ordinary multi-member gzip and which callVar inflates on the GPU."""
import argparse

from . import utils_v2


def reblock(src, dst, level=6):
    """-> bytes of text written"""
    proc, fo = utils_v2._open_tensor_stream(src)
    total, done = 0, False
    try:
        with utils_v2.BgzfWriter(dst, level=level) as out:
            while True:
                chunk = fo.read(1 << 24)
                if not chunk:
                    break
                total += out.write(chunk)
        done = True
    finally:
        utils_v2._close_quietly_unless(done, proc, fo, src)
    return total


def main():
    parser = argparse.ArgumentParser(description="Rewrite a text tensor file (plain or gzip) as BGZF")
    parser.add_argument("src", help="input tensor file, PIPE for standard input")
    parser.add_argument("dst", help="output BGZF file")
    parser.add_argument("--level", type=int, default=6, help="zlib compression level, default: %(default)d")
    args = parser.parse_args()
    reblock(args.src, args.dst, args.level)


if __name__ == "__main__":
    main()
