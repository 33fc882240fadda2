"""Compress every episode of a dataset directory (the reference's compress_data.py), the frames encoded on the device:

    python3 compress_data.py --dataset_dir <dir>            ->  <dir>_compressed/<episode>.npz

Each camera frame becomes the JPEG file cv2 / PIL writes for it at --quality (default 50, the reference's) and --subsampling
(default 420, cv2's); how the result differs from the reference script's is in actmi.episode_compress."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main(argv=None):
    parser = argparse.ArgumentParser(description="Compress all episode files in a directory.")
    parser.add_argument("--dataset_dir", action="store", type=str, required=True, help="Directory containing the uncompressed datasets.")
    parser.add_argument("--quality", type=int, default=50, help="JPEG quality, 1..100")
    parser.add_argument("--subsampling", choices=("420", "444"), default="420", help="chroma subsampling")
    parser.add_argument("--device", type=str, default=None, help="the device that encodes (default: the current one)")
    args = parser.parse_args(argv)
    from actmi.data import compress_dataset_dir
    written = compress_dataset_dir(args.dataset_dir, quality=args.quality, mode=args.subsampling, device=args.device)
    print(f"{len(written)} episodes compressed into {args.dataset_dir.rstrip('/')}_compressed")


if __name__ == "__main__":
    main()
