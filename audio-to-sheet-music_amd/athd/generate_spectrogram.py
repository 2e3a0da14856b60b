"""`generate_spectrogram.py` twin: the spectrogram arrays of one or more MUSDB18 test tracks, on the native hot path.

    python -m athd.generate_spectrogram "Tom McKenzie - Directions" --test-dir DIR --config config.yaml
    python -m athd.generate_spectrogram --top5 --test-dir DIR --output-dir results/spectrograms

Mirrors, name for name:
  * `TOP5_TRACKS`    <- `generate_spectrogram.py:21-27`.
  * `process_track`  <- `:30-104`: separate all stems, trim everything to the common length (`:52-60`), the
                        all-stems set and one mixture / estimate / ground-truth set per stem.  The arrays a figure
                        would show are saved as `.npz` under the reference's file names (no figure is drawn, no wandb):
                          <safe>_all_stems.npz   {stem}_estimated, {stem}_reference, vmin, vmax, extent
                          <safe>_<stem>.npz      mixture, estimated, reference, titles, vmin, vmax, extent
  * `main`           <- `:107-175`; the test and output directories, which the reference hard-codes, are arguments and
                        the checkpoint is the config's `wandb.checkpoint_dir/best_model.pt`, as in `athd.inference.main`.
Tracks come from `athd.musdb.MusDBTracks` (the decoded forms), not from `.stem.mp4`.
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

from .benchmark import SAMPLE_RATE, OurModel
from .musdb import MusDBTracks
from .utils import all_stems_npz, all_stems_spectrograms, separation_spectrograms
from .weights import STEMS

# Top 5 tracks by average SDR (generate_spectrogram.py:21-27)
TOP5_TRACKS = [
    "Speak Softly - Like Horses",
    "Tom McKenzie - Directions",
    "BKS - Too Much",
    "Lyndsey Ollard - Catching Up",
    "The Mountaineering Club - Mallory",
]


def process_track(track_name: str, model: OurModel, tracks: MusDBTracks, output_dir) -> bool:
    """`generate_spectrogram.py:30-104`: False (and nothing written) if `tracks` has no track of that name."""
    names = [tracks.name(i) for i in range(len(tracks))]
    if track_name not in names:
        print(f"Track not found: {tracks.root / track_name}")
        return False
    print(f"\n{'=' * 60}\nProcessing: {track_name}\n{'=' * 60}")
    print("Loading track...")
    _, mixture, reference_stems = tracks.track(names.index(track_name))
    print("Separating stems...")
    estimated_stems = model.separate_all(mixture)

    min_len = min(mixture.shape[-1], min(e.shape[-1] for e in estimated_stems.values()),
                  min(r.shape[-1] for r in reference_stems.values()))
    mixture = mixture[:, :min_len]
    estimated_stems = {k: v[:, :min_len] for k, v in estimated_stems.items()}
    reference_stems = {k: v[:, :min_len] for k, v in reference_stems.items()}

    print("Generating spectrograms...")
    output_dir = Path(output_dir)
    output_dir.mkdir(parents=True, exist_ok=True)
    safe_name = track_name.replace(" ", "_").replace("'", "")
    path = output_dir / f"{safe_name}_all_stems.npz"
    np.savez(path, **all_stems_npz(all_stems_spectrograms(mixture, estimated_stems, reference_stems, SAMPLE_RATE)))
    print(f"Saved: {path}")
    for stem in STEMS:
        d = separation_spectrograms(mixture, estimated_stems[stem], reference_stems[stem], stem, SAMPLE_RATE)
        mix, est, ref = (a.cpu().numpy() for a in d["spectrograms"].values())
        path = output_dir / f"{safe_name}_{stem}.npz"
        np.savez(path, mixture=mix, estimated=est, reference=ref, titles=np.array(list(d["spectrograms"])),
                 vmin=np.float32(d["vmin"]), vmax=np.float32(d["vmax"]), extent=np.asarray(d["extent"]))
        print(f"Saved: {path}")
    return True


def main(argv=None) -> int:
    import argparse

    from .inference import load_config, load_model
    ap = argparse.ArgumentParser(prog="python -m athd.generate_spectrogram",
                                 description="Generate spectrogram arrays for one or more tracks")
    ap.add_argument("track_names", nargs="*", help="track name(s) as the test directory lists them")
    ap.add_argument("--top5", action="store_true", help="process all top 5 tracks by SDR")
    ap.add_argument("--test-dir", default="../musdb18/test")
    ap.add_argument("--config", default="config.yaml")
    ap.add_argument("--output-dir", default="results/spectrograms")
    args = ap.parse_args(argv)
    track_names = TOP5_TRACKS if args.top5 else (args.track_names or ["Tom McKenzie - Directions"])
    print(f"Will process {len(track_names)} track(s):")
    for t in track_names:
        print(f"  - {t}")
    checkpoint = str(Path(load_config(args.config)["wandb"]["checkpoint_dir"]) / "best_model.pt")
    tracks = MusDBTracks(args.test_dir)
    print("Loading model...")
    model = OurModel(load_model(checkpoint))
    successful = sum(bool(process_track(t, model, tracks, args.output_dir)) for t in track_names)
    print(f"\n{'=' * 60}\nDone! Processed {successful}/{len(track_names)} tracks\n"
          f"Spectrograms saved to: {args.output_dir}\n{'=' * 60}")
    return 0 if successful == len(track_names) else 1


if __name__ == "__main__":
    sys.exit(main())
