"""Feature extraction behind the reference's front ends (reference multimodal/features/): `hac`, the histograms of acoustic
co-occurrences from frame streams on."""
