"""kmer_spans_amd -- MI355X-native k-mer span scanner (drop-in for the
span-scan path of lmjakt/kmer_spans).

Public API mirrors kmer_spans.R: kmer_counts, kmer_regions,
kmer_low_comp_regions, kmer_seq; score tables log2_table, pm1_table,
rank_table; per-region spectra and entropy region_spectra, their pairwise
distances region_distances, the tree of those region_hclust and its groups
cut_tree, the neighbour-joining tree region_nj with nj_edges and nj_newick,
the principal components of the spectra region_pca, the silhouette
widths, medoids and diameters of a tree cut region_silhouette, and, without
any distance matrix, the group mean spectra of a labelling
region_group_means, Lloyd k-means of the spectra region_kmeans, its maximin
and k-means++ starts region_kmeans_seed and the k nearest regions of every
region region_knn.
Device-resident entry points live in
kmer_spans_amd.device.
All results come from libkmerspans.so (HIP, gfx950); there is no CPU path.
"""
from ._lib import KmerSpansError, LIB_PATH, context  # noqa: F401
from .api import (kmer_counts, kmer_low_comp_regions, kmer_regions, kmer_seq,  # noqa: F401
                  kmer_magic, kmers_to_file, log2_table, lr_regions, pm1_table, rank_table, read_fasta,
                  read_kmers, region_distances, region_hclust, region_spectra, cut_tree, set_devices, get_devices,
                  window_kmer_dist, write_kmers, region_nj, nj_edges, nj_newick, region_pca, region_silhouette,
                  region_kmeans, region_group_means, region_knn, region_kmeans_seed)

__all__ = ["kmer_counts", "kmer_regions", "kmer_low_comp_regions", "kmer_seq", "lr_regions", "log2_table",
           "pm1_table", "rank_table", "kmer_magic", "kmers_to_file", "read_kmers", "write_kmers", "read_fasta",
           "window_kmer_dist", "region_spectra", "region_distances", "region_hclust", "cut_tree", "region_nj", "nj_edges", "nj_newick", "region_pca", "region_silhouette",
           "region_kmeans", "region_group_means", "region_knn", "region_kmeans_seed",
           "set_devices", "get_devices", "KmerSpansError",
           "context"]
