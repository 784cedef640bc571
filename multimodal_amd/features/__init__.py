"""Feature extraction behind the reference's front ends (reference multimodal/features/): `mfcc`, audio to cepstra and deltas;
`hac`, the histograms of acoustic co-occurrences from frame streams (or audio) on; `codebook`; `angle_histograms`."""
