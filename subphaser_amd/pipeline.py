"""`subphaser` command line for modules 1-2 and parts of 3-4: ingest -> count -> matrix/filter -> cluster (PCA, heatmap)
-> bin map -> window enrichment -> custom features -> homoeologous blocks -> LTR-RTs, on the MI355X hot path.

What is kept from the reference is its CONTRACT: the flag surface (subphaser/__main__.py:29-248), the names
and formats of the files under `-o` / `-tmpdir` and the checkpoint files, so that
modules 3-4 of the reference (LTR, circos) and existing command lines keep working on these outputs.
How the run is organised is this build's own: one option record (the `CLI` table's defaults under the caller's
options: a stage reads `self.<option>`, never a default of its own), a `Layout` that owns every path, seven
stages with explicit inputs and outputs (stage_ingest, stage_count_filter, stage_cluster, stage_windows,
stage_features, stage_blocks, stage_ltr), one queue of writers and figures that finish on the main thread, and a
second half that never leaves the device between the bin map, the window stack and the Fisher tests --
`.subgenome.bin.count` is written FROM the device arrays as an output, it is not parsed back (the reference
re-reads it with Circos.stack_matrix before it can enrich).

Of modules 3-4 one step is here: the homoeologous blocks of the circos figure's innermost ring (step_blocks,
__main__.py:699-713).  The reference runs an aligner on every pair of homoeologous chromosomes; stage_blocks votes
over the single-copy k-mers two chromosomes share, on the packed genome the map stage has just walked (blocks.py,
csrc/sp_blocks.hip), and writes `blocks.tsv`, `block_link.txt` (the format of Circos.paf2blocks) and a figure.  It
runs unless -just_core, -disable_circos or -disable_blocks is given.

Of module 3 the part that needs no detector is here: stage_ltr takes LTR-RT coordinates from -ltr_scn (the `.scn` the
reference's LTR step writes), maps the subgenome-specific k-mers onto the elements of the resident genome, writes
`.ltr.bin.count`, `.ltr.enrich`, `.ltr.identity.tsv`, `.ltr.insert.data` / `.summary` and the two age figures; the
divergence of an element's two LTRs comes from a banded alignment on the device (ltr.py, csrc/sp_ltralign.hip).  With
-ltr_denovo instead of -ltr_scn the coordinates are detected on the resident genome first (csrc/sp_ltrdetect.hip: exact
seeds, gapless extension; ltr.detect: the loop over the chromosomes and the chaining) and written as `.ltr.scn`.  With
-ltr_tree the subgenome-specific elements get ONE tree of this build's own: MinHash sketches and neighbour joining on the
device (ltrtree.py, csrc/sp_ltrtree.hip), `.ltr.tree.nwk` / `.map` and a figure.  With -ltr_hmm the records are classified
from the protein domains of their inner sequences first (domains.py, csrc/sp_domains.hip: this build's own Viterbi search of the
user's profile HMMs, TEsorter's rules behind it): `.ltr.dom.gff3`, `.ltr.cls.tsv`, records that are no LTR-RTs dropped;
-ltr_dom_prefilter searches only the (frame, profile) pairs whose best ungapped segment reaches a threshold (a heuristic).  With
-ltr_domtree (and -ltr_hmm) the subgenome-specific elements that have all of -ltr_domains get one tree per Copia / Gypsy from
their domains (domtree.py, csrc/sp_domalign.hip: this build's own profile alignment, occupancy trimming, Kimura distances and
neighbour joining): `.ltr.cls.pep` and `.ltr.LTR_<Superfamily>.aln` / `.map` / `.aln.trimmed` / `.aln.rooted.tre` and a figure.
ltr_finder / ltrharvest themselves, TEsorter, mafft / trimal / iqtree and the circos figure itself stay with the reference.
"""
import argparse
import io
import math
import os
import pickle
import shutil
import time
import sys
from collections import Counter, OrderedDict

import numpy as np

from . import REFERENCE_VERSION, __version__
from . import blocks as blocks_mod
from . import domains as domains_mod
from . import ltr as ltr_mod
from . import domtree as domtree_mod
from . import ltrtree as ltrtree_mod
from . import circos, seqs, stats
from .cluster import BOOTSTRAP_ENGINES, TEST_METHODS, Cluster
from .config import SGConfig, check_duplicates, parse_idmap
from .jellyfish import JellyfishDumps, plot_histogram, run_jellyfish_dumps
from .runtime import get_context, logger

NCPU = len(os.sched_getaffinity(0))
BIN_SIZE, CHUNK_SIZE, FEATURE_BIN = 10000, 10_000_000, 10_000_000   # Seqs.map_kmer3 defaults / __main__.py:509

# ---------------------------------------------------------------------------------------------------- CLI
# (group title, group description, [(flags, argparse keywords)]) -- the reference's options for modules 1-2;
# options of modules 3-4 are accepted (and ignored) so that one command line serves both programs.
_STR = dict(type=str, metavar="STR", default=None)
_FLAG = dict(action="store_true", default=False)
CLI = [
    ("Input", "Input genome and config files", [
        (("-i", "-genomes"), dict(dest="genomes", nargs="+", metavar="GENOME", required=True)),
        (("-c", "-sg_cfgs"), dict(dest="sg_cfgs", nargs="+", metavar="CFGFILE", required=True)),
        (("-labels",), dict(nargs="+", type=str, metavar="LABEL")),
        (("-no_label",), _FLAG),
        (("-target",), dict(type=str, metavar="FILE", default=None)),
        (("-sg_assigned",), dict(type=str, metavar="FILE", default=None)),
        (("-sep",), dict(type=str, metavar="STR", default="|")),
        (("-custom_features",), dict(nargs="+", metavar="FASTA|BED", default=None,
                                     help="feature sets to test for subgenome enrichment: FASTA files of feature sequences "
                                          "(ids chrom:start-end, as the reference takes them) and / or BED files of "
                                          "intervals on the target chromosomes (reduced over the resident genome: no "
                                          "sequence is uploaded)")),
    ]),
    ("Output", None, [
        (("-pre", "-prefix"), dict(dest="prefix", metavar="STR", default=None)),
        (("-o", "-outdir"), dict(dest="outdir", metavar="DIR", default="phase-results")),
        (("-tmpdir",), dict(type=str, metavar="DIR", default="tmp")),
        (("-colors",), dict(dest="colors", metavar="HEX,HEX[,...]", default=None)),
    ]),
    ("Kmer", "Options to count and filter kmers", [
        (("-k",), dict(type=int, metavar="INT", default=15)),
        (("-f", "-min_fold"), dict(dest="min_fold", type=float, metavar="FLOAT", default=2)),
        (("-q", "-min_freq"), dict(dest="min_freq", type=int, metavar="INT", default=200)),
        (("-baseline",), dict(type=int, default=1)),
        (("-ratio",), dict(type=float, default=1)),
        (("-lower_count",), dict(type=int, metavar="INT", default=3)),
        (("-min_prop",), dict(type=float, metavar="FLOAT", default=None)),
        (("-max_freq",), dict(type=int, metavar="INT", default=1e9)),
        (("-max_prop",), dict(type=float, metavar="FLOAT", default=None)),
        (("-low_mem",), dict(action="store_true", default=None)),
        (("-by_count",), dict(help="parsed, never used: as in the reference (__main__.py:98 vs :422-426)", **_FLAG)),
        (("-re_filter",), _FLAG),
    ]),
    ("Cluster", "Options for clustering to phase", [
        (("-nsg",), dict(type=int, metavar="INT", default=None)),
        (("-replicates",), dict(type=int, metavar="INT", default=1000)),
        (("-jackknife",), dict(type=float, metavar="FLOAT", default=50)),
        (("-max_pval",), dict(type=float, metavar="FLOAT", default=0.05)),
        (("-test_method",), dict(choices=list(TEST_METHODS), default="ttest_ind")),
        (("-figfmt",), dict(type=str, choices=["pdf", "png"], default="pdf")),
        (("-heatmap_colors",), dict(nargs="+", metavar="COLOR", default=("green", "black", "red"))),
        (("-heatmap_options",), dict(metavar="STR", default="", help="R syntax for heatmap.2 in the reference; the figure "
                                     "is drawn here without R, so a value is accepted, warned about and ignored")),
        (("-heatmap_size",), dict(type=int, metavar="INT", default=10000,
                                  help="k-mers sampled for the clustered heatmap (the reference's constant); 0: no heatmap")),
        (("-just_core",), _FLAG),
    ]),
    ("LTR / Circos", "accepted for command-line compatibility; modules 3-4 stay with the reference, except the homoeologous "
                     "blocks (-disable_blocks, -min_block, -alt_cfgs are used; see Blocks) and the LTR stage on given coordinates "
                     "(-disable_ltr, -mu, -exclude_exchanges, -non_specific are used; see LTR)",
     [((o,), _STR) for o in ("-ltr_finder_options", "-ltr_harvest_options", "-tesorter_options", "-trimal_options",
                             "-tree_method", "-tree_options", "-ggtree_options", "-aligner", "-aligner_options",
                             "-chr_ordered")]
     + [((o,), dict(nargs="+", default=None)) for o in ("-ltr_detectors", "-ltr_domains", "-alt_cfgs")]
     + [((o,), _FLAG) for o in ("-disable_ltr", "-all_ltr", "-intact_ltr", "-exclude_exchanges", "-non_specific",
                                "-disable_ltrtree", "-disable_circos", "-disable_blocks")]
     + [(("-mu",), dict(type=float, default=13e-9)), (("-subsample",), dict(type=int, default=ltrtree_mod.SUBSAMPLE)),
        (("-window_size",), dict(type=int, metavar="INT", default=1000000)),
        (("-min_block",), dict(type=int, default=blocks_mod.MIN_BLOCK,
                               help="shortest homoeologous block (span on the first chromosome of the pair) that is kept"))]),
    ("Blocks", "homoeologous blocks from shared single-copy k-mers (replaces the aligner of the reference's step_blocks; "
               "-aligner / -aligner_options are accepted and run nothing).  The defaults are provisional", [
        (("-block_k",), dict(type=int, metavar="INT", default=blocks_mod.BLOCK_K, help="anchor k-mer size, odd, 17..31")),
        (("-block_sample",), dict(type=int, metavar="INT", default=blocks_mod.BLOCK_SAMPLE,
                                  help="one k-mer in 2^INT is an anchor candidate (0..16)")),
        (("-block_bin",), dict(type=int, metavar="INT", default=blocks_mod.BLOCK_BIN, help="voting window in bases")),
        (("-block_votes",), dict(type=int, metavar="INT", default=blocks_mod.BLOCK_VOTES,
                                 help="anchors the winning cell of a window needs for the window to be called")),
        (("-block_gap",), dict(type=int, metavar="INT", default=blocks_mod.BLOCK_GAP,
                               help="windows a block may skip, and drift off its diagonal, between two called windows")),
    ]),
    ("LTR", "subgenome-specific LTR-RTs and their insertion ages from LTR-RT coordinates (the reference's module 3 without "
            "TEsorter itself and the LTR trees): the stage runs when -ltr_scn or -ltr_denovo is given, unless -just_core or "
            "-disable_ltr; without -ltr_hmm every record is used, as under -all_ltr; -mu, -exclude_exchanges and -non_specific are honoured; "
            "-ltr_tree adds this build's own tree of the subgenome-specific elements (-subsample and -disable_ltrtree are used); "
            "-ltr_hmm classifies the records from protein domains and drops those that are no LTR-RTs (-all_ltr keeps them); "
            "-ltr_domtree adds this build's own tree per Copia / Gypsy from the domains (-ltr_domains, -subsample, -disable_ltrtree are used)", [
        (("-ltr_scn",), dict(type=str, metavar="FILE", default=None,
                             help="LTR-RTs in the 12-column format of the reference's tmp/LTR.scn (ltrharvest's columns plus the "
                                  "sequence id)")),
        (("-ltr_identity",), dict(choices=list(ltr_mod.IDENTITY_MODES), default="align",
                                  help="divergence of an element's two LTRs: align (banded global alignment on the GPU, "
                                       "mismatch / (match + mismatch)) or scn (1 - similarity / 100 of the file, as the reference)")),
        (("-ltr_band",), dict(type=int, metavar="INT", default=ltr_mod.LTR_BAND,
                              help="diagonals either side of the band of the LTR alignment; provisional: judged on synthetic pairs only")),
        (("-ltr_denovo",), dict(help="detect the LTR-RTs on the GPU (exact seeds at a bounded distance, gapless X-drop extension, "
                                     "chaining; no TSD or motif search) and write them to `.ltr.scn`; not with -ltr_scn.  The "
                                     "defaults of the -ltr_* options below are the values the reference passes to its detectors "
                                     "and are provisional: judged on synthetic genomes only, never against ltrharvest or "
                                     "ltr_finder", **_FLAG)),
        (("-ltr_seed",), dict(type=int, metavar="INT", default=ltr_mod.LTR_SEED, help="length of the exact seed, 12..20")),
        (("-ltr_mindist",), dict(type=int, metavar="INT", default=ltr_mod.LTR_MINDIST, help="smallest distance between the starts of the two LTRs")),
        (("-ltr_maxdist",), dict(type=int, metavar="INT", default=ltr_mod.LTR_MAXDIST, help="largest such distance, at most 32767")),
        (("-ltr_minlen",), dict(type=int, metavar="INT", default=ltr_mod.LTR_MINLEN, help="shortest LTR")),
        (("-ltr_maxlen",), dict(type=int, metavar="INT", default=ltr_mod.LTR_MAXLEN, help="longest LTR, at most 8192")),
        (("-ltr_xdrop",), dict(type=int, metavar="INT", default=ltr_mod.LTR_XDROP, help="X-drop of the gapless extension (+2 / -2)")),
        (("-ltr_similar",), dict(type=float, metavar="FLOAT", default=ltr_mod.LTR_SIMILAR,
                                 help="minimum similarity of the two LTRs in percent: match / (match + mismatch + gap) of their alignment")),
        (("-ltr_chain_indel",), dict(type=int, metavar="INT", default=ltr_mod.LTR_CHAIN_INDEL,
                                     help="chaining: largest shift of the diagonal between two extended seeds")),
        (("-ltr_chain_join",), dict(type=int, metavar="INT", default=ltr_mod.LTR_CHAIN_JOIN,
                                    help="chaining: largest distance of an extended seed from the end of its chain")),
        (("-ltr_hmm",), dict(type=str, metavar="FILE", default=None,
                             help="classify the LTR-RTs from the protein domains of their inner sequences: profile HMMs in HMMER3 "
                                  "text format (REXdb's `.hmm` as TEsorter ships it, or any other) are searched in the six-frame "
                                  "translation on the GPU, and TEsorter's rules give order, superfamily and clade: "
                                  "`.ltr.dom.gff3`, `.ltr.cls.tsv`; records whose order is not LTR are dropped unless -all_ltr.  "
                                  "The search is this build's own integer Viterbi alignment, one hit per frame and profile, "
                                  "not hmmscan: no E-values")),
        (("-ltr_dom_cov",), dict(type=float, metavar="FLOAT", default=domains_mod.MIN_COV,
                                 help="minimum share of a profile's nodes a domain covers, in percent (TEsorter's 20)")),
        (("-ltr_dom_score",), dict(type=float, metavar="FLOAT", default=domains_mod.MIN_SCORE,
                                   help="minimum score of a domain in bits per node (TEsorter's 0.5); provisional: these bits are "
                                        "not HMMER's")),
        (("-ltr_dom_prefilter",), dict(type=float, nargs="?", metavar="BITS", const=domains_mod.PREFILTER_BITS, default=None,
                                       help="search only the (frame, profile) pairs whose best UNGAPPED segment scores at least "
                                            "BITS bits (needs -ltr_hmm; without a value: {}); absent: every pair is searched.  A "
                                            "heuristic that makes the search of many elements affordable: a domain whose best "
                                            "ungapped segment scores below BITS is lost.  This build's rule, not HMMER's P-value "
                                            "filter; the default is provisional".format(domains_mod.PREFILTER_BITS))),
        (("-ltr_tree",), dict(help="build ONE tree over the subgenome-specific LTR-RTs on the GPU and write `.ltr.tree.nwk`, "
                                   "`.ltr.tree.map` and `.ltr.tree.<figfmt>`: MinHash sketches of the elements' k-mers, Mash "
                                   "distances, neighbour joining, midpoint rooting.  Not a protein-domain tree and not one tree per "
                                   "Copia / Gypsy (nothing is classified); never compared with iqtree or FastTree.  Above roughly "
                                   "25-30 %% divergence at k = 13 the distances saturate, so unrelated families are joined in no "
                                   "meaningful order.  At most -subsample elements (0: all; 4096 at most), chosen with "
                                   "-bootstrap_seed; elements above 65536 bases are left out; -disable_ltrtree wins.  "
                                   "-ggtree_options, -tree_method, -tree_options, -trimal_options and -ltr_domains run nothing",
                              **_FLAG)),
        (("-ltr_tree_k",), dict(type=int, metavar="INT", default=ltrtree_mod.TREE_K,
                                help="k-mer size of the tree's sketches, odd, 9..31; provisional: judged on synthetic families only")),
        (("-ltr_tree_sketch",), dict(type=int, metavar="INT", default=ltrtree_mod.TREE_SKETCH,
                                     help="hashes per sketch, 16..4096; provisional: judged on synthetic families only")),
        (("-ltr_domtree",), dict(help="build one tree per Copia / Gypsy from the protein domains of the subgenome-specific "
                                      "LTR-RTs (needs -ltr_hmm): `.ltr.cls.pep`, and per superfamily `.ltr.LTR_<Superfamily>.aln`, "
                                      "`.map`, `.aln.trimmed`, `.aln.rooted.tre` and `.tree.<figfmt>`.  The elements with all of "
                                      "-ltr_domains (default INT RT RH) are aligned on the GPU to one profile per domain by this "
                                      "build's own Viterbi path, columns below -ltr_tree_occupancy are dropped, Kimura distances "
                                      "and neighbour joining give the tree.  Not mafft, trimal or iqtree, and never compared with "
                                      "them; inserted residues appear in no column.  At most -subsample elements (4096 at most) "
                                      "per tree; -disable_ltrtree wins; independent of -ltr_tree", **_FLAG)),
        (("-ltr_tree_occupancy",), dict(type=int, metavar="INT", default=domtree_mod.OCCUPANCY,
                                        help="percent of the rows that must hold a residue for a column of the domain alignment to "
                                             "stay; provisional")),
        (("-ltr_tree_overlap",), dict(type=int, metavar="INT", default=domtree_mod.OVERLAP,
                                      help="columns two rows of the domain alignment must share; below it their distance is the "
                                           "largest one; provisional")),
    ]),
    ("Other options", None, [
        (("-p", "-ncpu"), dict(dest="ncpu", type=int, metavar="INT", default=NCPU)),
        (("-max_memory",), dict(type=str, metavar="MEM", default=None)),
        (("-cleanup",), _FLAG),
        (("-overwrite",), _FLAG),
        (("-engine",), dict(type=int, default=0, help="k-mer counting engine (0 auto, 1 atomic table, 2 LDS radix, 3 LDS radix into lists: small genomes)")),
        (("-write_dumps",), dict(help="also write jellyfish-style text dumps {chrom}_{k}.fa", **_FLAG)),
        (("-bootstrap_seed",), dict(type=int, default=None, help="seed of k-means and of the bootstrap resampling")),
        (("-bootstrap_engine",), dict(choices=list(BOOTSTRAP_ENGINES), default="sklearn",
                                      help="k-means fits of the bootstrap: sklearn (the reference's loop of scikit-learn fits) or "
                                           "device (one kernel launch, greedy k-means++ and Lloyd per replicate; up to 128 "
                                           "chromosomes in 32 subgenomes, the scikit-learn loop beyond; the same -bootstrap_seed "
                                           "resamples the same k-mers under both)")),
    ]),
]


def option_defaults():
    """{dest: default} of every option of the `CLI` table: what the parser gives a command line that names none of them"""
    return {kw.get("dest", flags[0].lstrip("-")): kw.get("default") for _, _, options in CLI for flags, kw in options}


def makeArgparse(argv=None):
    parser = argparse.ArgumentParser(
        prog="subphaser", formatter_class=argparse.RawDescriptionHelpFormatter,
        description="Phase subgenomes of an allopolyploid or hybrid based on repetitive kmers "
                    "(MI355X-native k-mer counting / enrichment; modules 1-2 of SubPhaser).\n"
                    "Limits: 8 subgenome columns per config line unless -baseline is 1 or -1, 32 subgenomes in the "
                    "enrichment.  k = 9..15: any number of chromosomes (lists above 560), of which at most 1024 on config "
                    "lines of two or more units; singleton lines only add to the k-mer totals.  k <= 8: at most 560 "
                    "chromosomes.  k > 15: at most 1024 chromosomes in the filter.")
    for title, desc, options in CLI:
        group = parser.add_argument_group(title, desc)
        for flags, kw in options:
            group.add_argument(*flags, **kw)
    parser.add_argument("-v", "-version", action="version",
                        version="subphaser_amd {} (interface of SubPhaser {})".format(__version__, REFERENCE_VERSION))
    args = parser.parse_args(argv)
    if args.ltr_denovo and args.ltr_scn:
        parser.error("-ltr_denovo detects the LTR-RTs, -ltr_scn reads them from a file: give one of the two")
    if args.ltr_domtree and not args.ltr_hmm:
        parser.error("-ltr_domtree builds its trees from the domains of the classification: give -ltr_hmm FILE as well")
    if args.ltr_dom_prefilter is not None and not args.ltr_hmm:
        parser.error("-ltr_dom_prefilter filters the domain search of the classification: give -ltr_hmm FILE as well")
    if args.prefix is not None:          # the prefix goes in front of directory names AND file names (__main__.py:242-245)
        args.prefix = args.prefix.replace("/", "_")
        args.outdir, args.tmpdir = args.prefix + args.outdir, args.prefix + args.tmpdir
    return args


# ------------------------------------------------------------------------------------------- paths, checkpoints
class Layout:
    """Every path of a run.  `out("x")` = <outdir>/<prefix>k15_q200_f2.x, `ckp(name)` = <tmpdir>/<prefix>name.ok"""

    def __init__(self, outdir, tmpdir, prefix, k, min_freq, min_fold):
        self.outdir, self.tmpdir = os.path.realpath(outdir) + "/", os.path.realpath(tmpdir) + "/"
        os.makedirs(self.outdir, exist_ok=True)
        os.makedirs(self.tmpdir, exist_ok=True)
        self.out_prefix = self.outdir + (prefix or "")
        self.tmp_prefix = self.tmpdir + (prefix or "")
        self.basename = "k{}_q{}_f{}".format(k, min_freq, min_fold)

    def out(self, ext):
        return "{}{}.{}".format(self.out_prefix, self.basename, ext)

    def ckp(self, file_or_name):
        return "{}{}.ok".format(self.tmp_prefix, os.path.basename(file_or_name))

    @property
    def chromdir(self):
        return self.tmp_prefix + "chromosomes/"


def mk_ckp(ckpfile, *data):
    """A checkpoint is the objects pickled one after the other (the reference's small_tools.mk_ckp)."""
    with open(ckpfile, "wb") as f:
        for obj in data:
            pickle.dump(obj, f)
    logger.info("New check point file: `{}`".format(ckpfile))


def check_ckp(ckpfile):
    """False: no checkpoint.  True: an empty one.  Otherwise the list of objects it holds."""
    if not os.path.exists(ckpfile):
        return False
    logger.info("Check point file: `{}` exists; skip this step".format(ckpfile))
    objs = []
    with open(ckpfile, "rb") as f:
        while True:
            try:
                objs.append(pickle.load(f))
            except EOFError:
                break
    return objs or True


# ------------------------------------------------------------------------------------------------- the run
def _bg_min_rows():
    """outputs with at least this many rows are written on a background thread (SP_BG_MIN_ROWS: tests force it)"""
    return int(os.environ.get("SP_BG_MIN_ROWS", "200000"))


class Pipeline:
    # Every option is a CLASS attribute at its default of the `CLI` table (set below the class); an instance holds what its
    # caller gave.  So an object put together by hand -- Pipeline.__new__ and some attributes -- reads the parser's defaults
    # for the rest, too.
    _ltr_tree_built = False      # stage_ltr wrote a tree (it starts by putting this back): _run words its closing note by it
    _ltr_domtrees_built = ()     # the superfamilies whose domain tree stage_ltr wrote (-ltr_domtree), likewise
    _ltr_dominfo = None          # what _ltr_classify keeps for the domain trees: domains, class rows, inner intervals

    def _configure(self, opts):
        """the state of a run and the caller's options (the others are the class's defaults); -colors as a list or None"""
        self._reset()
        self.__dict__.update(opts)
        if isinstance(self.colors, str):
            self.colors = self.colors.split(",")

    def _reset(self):
        """the containers of a run's state"""
        self._background = []             # (name, wait, done) of the writers and figures that finish on the main thread
        self.d_targets = {}               # ids as they are in the input -> labels (stage_ingest)

    @classmethod
    def bare(cls, **over):
        """A pipeline with its options and nothing read: no genome, no config file.  For a single stage, and for tests."""
        p = cls.__new__(cls)
        p._configure(over)
        return p

    def __init__(self, genomes, sg_cfgs, labels=None, **opts):
        self._configure(opts)
        check_duplicates(genomes)
        check_duplicates(labels)
        self.genomes, self.sg_cfgs = genomes, sg_cfgs
        n = len(genomes)
        if self.no_label or (labels is None and n == 1):
            self.labels = [""] * n
        elif labels is None:
            self.labels = ["{}-".format(i) for i in range(1, n + 1)]
        else:
            self.labels = labels
        # one prefix per config file when the counts match, else none (__main__.py:274-281)
        cfg_prefix = self.labels if len(self.labels) == len(sg_cfgs) else [None] * len(sg_cfgs)
        cfgs = [SGConfig(f, prefix=p, sep=self.sep) for f, p in zip(sg_cfgs, cfg_prefix)]
        self.sgs = [line for cfg in cfgs for line in cfg.sgs]
        self.chrs = [c for cfg in cfgs for c in cfg.chrs]
        if not self.nsg or self.nsg < 2:
            self.nsg = sum(cfg.nsg for cfg in cfgs)

    # ---- stage 1: chromosomes ---------------------------------------------------------------------------
    def stage_ingest(self, lay):
        """Target chromosomes as per-chromosome FASTA (+ in-memory records); checkpoint `split.ok` holds
        (chromfiles, labels, d_targets, d_size) like the reference's."""
        logger.info("chromosomes named in the config: {}".format(self.chrs))
        logger.info("per-chromosome FASTA under `{}`".format(lay.chromdir))
        ckp = lay.ckp("split")
        saved = None if self.overwrite else check_ckp(ckp)
        reuse = isinstance(saved, list) and len(saved) == 4
        if reuse:
            chromfiles, labels, d_targets, d_size = saved
            if set(d_targets) != set(self.chrs):        # another target set: split again, and filter again
                reuse, self.re_filter = False, True
            elif not all(os.access(f, os.R_OK) for f in chromfiles):
                reuse = False
        if not reuse:
            # The per-chromosome copies are an OUTPUT for the reference's later modules; counting uses the records
            # in memory.  Their writer threads keep going while the GPU counts; `split.ok` is recorded once they
            # are done (_finish_background).
            os.makedirs(lay.chromdir, exist_ok=True)
            chromfiles, labels, d_targets, d_size, waiting = seqs.split_genomes(
                self.genomes, self.labels, self.chrs, lay.chromdir, d_targets=parse_idmap(self.target), sep=self.sep,
                defer=True)
            self._background.append(("chromosome files", waiting.wait,
                                     lambda: mk_ckp(ckp, chromfiles, labels, d_targets, d_size)))
        self.d_targets = dict(d_targets)      # ids as they are in the input -> labels (BED files may use either)
        # config order, not file order
        where = dict(zip(labels, chromfiles))
        labels = [lab for lab in d_targets.values() if lab in where]
        chromfiles = [where[lab] for lab in labels]
        if not chromfiles:
            raise ValueError("0 chromosome remained after filtering. Please check the inputs.")
        logger.info("{} chromosomes, in config order: {}".format(len(labels), labels))
        logger.info("Genome size: {:,} bp".format(sum(d_size.values())))
        rename = d_targets.get
        self.sgs = [[[rename(c, c) for c in unit] for unit in line] for line in self.sgs]
        logger.info("homoeologous sets after renaming: {}".format(self.sgs))
        assigned = {}
        if self.sg_assigned:
            for line in open(self.sg_assigned):
                if line.strip() and not line.startswith("#"):
                    c, sg = line.split()[:2]
                    assigned[rename(c, c)] = sg
        return chromfiles, labels, d_size, assigned

    # ---- stage 2: count + matrix + differential filter --------------------------------------------------
    def stage_count_filter(self, lay, chromfiles, labels):
        logger.info("###Step: Kmer Count")
        logger.info("Counting kmer on the GPU (replaces jellyfish)")
        dumpfiles = run_jellyfish_dumps(chromfiles, k=self.k, ncpu=self.ncpu, lower_count=self.lower_count,
                                        overwrite=self.overwrite, engine=self.engine, write_dumps=self.write_dumps)
        logger.info("chromosome x k-mer matrix: the count tables in HBM")
        dumps = JellyfishDumps(dumpfiles, labels, ncpu=self.ncpu)
        d_mat = dumps.to_matrix()
        logger.info("differential k-mer filter (K3)")
        histfig = lay.out("kmer_freq." + self.figfmt)
        d_mat2 = dumps.filter(d_mat, dumps.lengths, self.sgs, outfig=histfig, min_fold=self.min_fold,
                              baseline=self.baseline, min_freq=self.min_freq, max_freq=self.max_freq,
                              min_prop=self.min_prop, max_prop=self.max_prop, ratio=self.ratio)
        logger.info("{} kmers in total".format(len(d_mat)))
        if len(d_mat2) == 0:
            raise ValueError("0 kmer remained after filtering. Please reset the filter options.")
        # The matrix in memory is what every later stage uses, so the file always describes THIS run's filter:
        # it is rewritten whenever it is recomputed (an old file next to new calls would be inconsistent).
        # It is 0.5 GB of text at wheat scale: a writer thread (the library formats the rows on its own threads) works
        # while the clustering and mapping stages run; the checkpoint follows the writer's end.
        matfile = lay.out("kmer.mat")
        t0 = time.perf_counter()
        # the k-mer tests of the next stage read the rows on the device: copy them there now, while nothing else
        # competes for the host memory bus
        if getattr(d_mat2, "counts", None) is not None and getattr(d_mat2, "ctx", None) is not None \
                and hasattr(d_mat2.ctx, "stage_rows"):
            d_mat2.counts_dev = d_mat2.ctx.stage_rows(d_mat2.counts)
        self._write_matrix_in_background(dumps, d_mat2, matfile, histfig, lay)
        logger.info("`{}` + histogram figure: writer started in {:.2f} s".format(os.path.basename(matfile),
                                                                             time.perf_counter() - t0))
        return d_mat2

    def _write_matrix_in_background(self, dumps, d_mat2, matfile, histfig, lay):
        tot = dumps.hist_tot()          # device -> host here: the writer thread makes no GPU calls

        def work(fout):
            dumps.write_matrix(d_mat2, fout)

        def done():
            # The figure is drawn on the MAIN thread, after the writers: importing matplotlib's extension modules
            # (dlopen under the GIL) on a writer thread while scikit-learn's threadpoolctl walks the loaded
            # libraries (dl_iterate_phdr calling back into Python) on a bootstrap thread is a lock-order deadlock
            # -- one wheat-scale run in four hung there.
            mk_ckp(lay.ckp(matfile))
            try:
                plot_histogram(tot, histfig)
            except Exception as e:     # the figure is optional
                logger.warning("histogram not plotted: {}".format(e))
        self._write_in_background(matfile, work, len(d_mat2) >= _bg_min_rows(), done=done)

    def _write_in_background(self, path, write, big, done=None):
        """write(fout) into `path`: on a thread of this process when the output is large (the library's text writers
        release the GIL and use their own threads; no child processes: the GPU process stays single), inline otherwise;
        `done` (e.g. the checkpoint) runs on the main thread once the file is complete.  `write` must not import
        anything (see _write_matrix_in_background)."""
        import threading
        done = done or (lambda: None)
        failure = []

        def work():
            try:
                with open(path, "w") as fout:
                    write(fout)
            except BaseException as e:      # re-raised by wait()
                failure.append(e)

        if not big:
            work()
            if failure:
                raise failure[0]
            done()
            return
        th = threading.Thread(target=work, name="writer:" + os.path.basename(path), daemon=False)
        th.start()

        def wait():
            th.join()
            if failure:
                raise failure[0]
        self._background.append((path, wait, done))

    def _finish_background(self):
        """Wait for the writers started along the way, then record their checkpoints.  A checkpoint describes ITS
        file only: run() also calls this after a later stage raised, and a `.kmer.mat` that was written completely
        keeps its checkpoint then (the file is valid; a rerun recomputes whatever depends on the failed stage)."""
        pending, self._background = self._background, []
        err = None
        for name, wait, done in pending:
            try:
                wait()
                done()
            except Exception as e:      # keep waiting for the others; report the first failure
                logger.error("background writer of {} failed: {}".format(name, e))
                err = err or e
        if err is not None:
            raise err

    def _plot_later(self, lay, what, figs, draw):
        """Queue draw() for the MAIN thread, behind the writers (why not a writer thread: _write_matrix_in_background).
        Each of `figs` that exists afterwards gets its checkpoint; a figure is optional: any failure is a warning."""
        def done():
            try:
                draw()
                for fig in figs:
                    if os.path.exists(fig):
                        mk_ckp(lay.ckp(fig))
            except Exception as e:
                logger.warning("{} not plotted: {}".format(what, e))
        self._background.append((figs[0], lambda: None, done))

    def _sg_colors(self, sg_names):
        """{subgenome: colour} from -colors, in the order of the names; None without -colors: the figure's own cycle"""
        return {sg: self.colors[i % len(self.colors)] for i, sg in enumerate(sg_names)} if self.colors else None

    # ---- stage 3: subgenome assignment + subgenome-specific k-mers --------------------------------------
    def stage_cluster(self, lay, d_mat2, assigned):
        logger.info("###Step: Cluster")
        cl = Cluster(d_mat2, n_clusters=self.nsg, sg_prefix="SG", sg_assigned=assigned, bootstrap=True,
                     replicates=self.replicates, jackknife=self.jackknife, seed=self.bootstrap_seed,
                     bootstrap_engine=self.bootstrap_engine)
        logger.info("Subgenome assignments: {}".format(dict(cl.d_sg)))
        with open(lay.out("chrom-subgenome.tsv"), "w") as fout:
            cl.output_subgenomes(fout)
        self._pca(lay, cl)      # before output_kmers: that releases the rows staged on the device
        sg_kmers = lay.out("sig.kmer-subgenome.tsv")
        logger.info("subgenome-specific k-mers -> `{}`".format(sg_kmers))
        t0 = time.perf_counter()
        kmer_labels, write = cl.output_kmers(None, max_pval=self.max_pval, test_method=self.test_method, defer=True)
        t1 = time.perf_counter()
        self._write_in_background(sg_kmers, write, len(kmer_labels.keys) >= _bg_min_rows())
        logger.info("k-mer tests {:.2f} s, text writer started in {:.2f} s".format(t1 - t0, time.perf_counter() - t1))
        self._heatmap(lay, cl, kmer_labels)      # after output_kmers: it colours the k-mers by their labels (host data only)
        per_sg = np.bincount(kmer_labels.sg_idx, minlength=len(kmer_labels.sg_names))
        logger.info("{} significant subgenome-specific kmers".format(len(kmer_labels.keys)))
        for sg, n in zip(kmer_labels.sg_names, per_sg.tolist()):
            if n:
                logger.info("\t{} {}-specific kmers".format(n, sg))
        return cl, kmer_labels

    def _pca(self, lay, cl):
        """`.kmer_pca.tsv` and `.kmer_pca.<figfmt>` (__main__.py:467-469).  The coordinates are written here, the figure
        with the background writers (drawn on the main thread, see _write_matrix_in_background).  Only non-finite input
        stops the run, as it would stop scikit-learn; any other failure costs these two files and nothing else."""
        if len(cl.chrs) < 2:
            logger.info("k-mer PCA skipped: {} chromosome".format(len(cl.chrs)))
            return
        tsv, fig = lay.out("kmer_pca.tsv"), lay.out("kmer_pca." + self.figfmt)
        t0 = time.perf_counter()
        try:
            draw = cl.pca(outfig=fig, outtsv=tsv, n_components=self.nsg or cl.n_clusters, colors=self.colors,
                          defer=True)
        except Exception as e:
            if isinstance(e, ValueError) and str(e).startswith("Input contains NaN or infinity"):
                raise
            logger.warning("k-mer PCA not written: {}".format(e))
            return
        mk_ckp(lay.ckp(tsv))
        logger.info("k-mer PCA ({}) -> `{}` in {:.2f} s".format(cl.pca_engine, os.path.basename(tsv), time.perf_counter() - t0))
        self._plot_later(lay, "k-mer PCA", [fig], draw)

    def _heatmap(self, lay, cl, kmer_labels):
        """`.kmer.mat.heatmap.tsv` and `.kmer.mat.<figfmt>` (the reference's figure name, __main__.py:461-464).  The table
        is written here, the figure with the background writers (drawn on the main thread, as the PCA's).  Only a wrong
        number of -heatmap_colors stops the run, as it stops the reference; any other failure costs these two files."""
        if self.heatmap_options:
            logger.warning("-heatmap_options is R syntax for heatmap.2; the heatmap is drawn without R and ignores `{}`".format(
                self.heatmap_options))
        if self.heatmap_size is None or self.heatmap_size <= 0:
            logger.info("heatmap skipped: -heatmap_size {}".format(self.heatmap_size))
            return
        if len(cl.chrs) < 2:
            logger.info("heatmap skipped: {} chromosome".format(len(cl.chrs)))
            return
        from .heatmap import check_colors
        panel = check_colors(self.heatmap_colors)      # ValueError: stops the run
        tsv, fig = lay.out("kmer.mat.heatmap.tsv"), lay.out("kmer.mat." + self.figfmt)
        t0 = time.perf_counter()
        try:
            draw = cl.heatmap(kmer_labels, outfig=fig, outtsv=tsv, size=self.heatmap_size, colors=self.colors,
                              heatmap_colors=panel, defer=True)
        except Exception as e:
            logger.warning("heatmap not written: {}".format(e))
            return
        if cl.heatmap_engine is None:      # fewer than 2 usable k-mers: logged there
            return
        mk_ckp(lay.ckp(tsv))
        logger.info("heatmap ({}) -> `{}` in {:.2f} s".format(cl.heatmap_engine, os.path.basename(tsv), time.perf_counter() - t0))
        self._plot_later(lay, "heatmap", [fig], draw)

    # ---- stage 4: bin map -> window stack -> enrichment, on the device -----------------------------------
    def stage_windows(self, lay, chromfiles, labels, d_size, cl, kmer_labels):
        ctx = get_context()
        S, names = len(cl.sg_names), cl.sg_names
        lengths = [d_size[lab] for lab in labels]
        sg_map = lay.out("subgenome.bin.count")
        logger.info("10-kb bin counts -> `{}`".format(sg_map))
        ctx.labels_set(kmer_labels.keys, kmer_labels.sg_idx, S)
        slots, n_mapped = ctx.map_bins_all(BIN_SIZE, CHUNK_SIZE)
        with open(sg_map, "w") as fout:     # an OUTPUT of the device arrays; nothing below reads it
            fout.write("\t".join(["#chrom", "start", "end"] + names) + "\n")
            for lab, n, sl in zip(labels, lengths, slots):
                seqs._write_lines(fout, lab, *seqs.bin_lines(lab, n, sl, BIN_SIZE, CHUNK_SIZE, self.k))
        mk_ckp(lay.ckp(sg_map))
        n_chunks = [max(1, -(-n // CHUNK_SIZE)) for n in lengths]
        hit = sum(c for c, m in zip(n_chunks, n_mapped.tolist()) if m)
        logger.info("Processed {} sequences".format(sum(n_chunks)))
        logger.info("{} ({:.2%}) sequences contain subgenome-specific kmers".format(hit, hit / max(1, sum(n_chunks))))
        if len(kmer_labels.keys):
            logger.info("{:.2%} of {} subgenome-specific kmers are mapped".format(
                ctx.labels_hit() / len(kmer_labels.keys), len(kmer_labels.keys)))
        logger.info("window enrichment, {}-bp windows (K6)".format(self.window_size))
        ws = int(self.window_size)
        win, woff, pvals, argmin, sig, ratios = ctx.stack_enrich(BIN_SIZE, CHUNK_SIZE, ws, lengths, self.max_pval, 0.5)
        nz = np.flatnonzero(win.any(axis=1))       # only windows that received a bin line exist (Circos.py:734-742)
        chrom = np.searchsorted(woff, nz, side="right") - 1
        rows = [(labels[c], int(w) * ws, int(w) * ws + ws) for c, w in zip(chrom.tolist(), (nz - woff[chrom]).tolist())]
        bin_enrich = lay.out("bin.enrich")
        with open(bin_enrich, "w") as f1, open(lay.out("bin.group"), "w") as f2:
            self.sg_lines = stats.enrich_bin(f1, f2, cl.d_sg, win[nz].astype(np.int64), colnames=names, rownames=rows,
                                             max_pval=self.max_pval,
                                             results=(pvals[nz], argmin[nz], sig[nz].astype(bool), ratios[nz]))
        logger.info("wrote {}".format(bin_enrich))

    # ---- stage 5: custom feature sets ----------------------------------------------------------------------
    def stage_features(self, lay, cl, kmer_labels):
        feat_map = lay.out("custom.bin.count")
        logger.info("feature sets: {}".format(self.custom_features))
        lines = []       # the written lines as arrays: `custom.bin.count` is an output, nothing below parses it back
        ivals = []       # BED feature sets: (IntervalRows, counts) per file, one row per feature
        beds = [f for f in self.custom_features if seqs.is_bed(f)]
        fastas = [f for f in self.custom_features if f not in beds]
        with open(feat_map, "w") as fout:
            if fastas or not beds:
                seqs.map_kmer3(fastas, kmer_labels, fout=fout, k=self.k, bin_size=FEATURE_BIN,
                               sg_names=cl.sg_names, chunk=False, log=False, collect=lines)
            if beds:
                # intervals: a reduction over the genome the GPU already holds; ids are synthesised as chrom:start-end
                # (what enrich_ltr's id rule expects); BED names may be the ids before or after renaming
                sub = io.StringIO() if fastas else fout      # behind FASTA lines: without a second header line
                seqs.map_intervals(beds, kmer_labels, {lab: i for i, lab in enumerate(self.labels)}, fout=sub, k=self.k,
                                   bin_size=FEATURE_BIN, sg_names=cl.sg_names, collect=ivals, aliases=dict(self.d_targets))
                if fastas:
                    fout.write(sub.getvalue().split("\n", 1)[1])      # one header line per file
        logger.info("feature enrichment")
        S = len(cl.sg_names)
        ids, counts = [], []
        if lines:
            names, code = circos.factorize_first([x for part in lines for x in part[0]])
            ids, counts = circos.stack_arrays(names, code, np.concatenate([part[1] for part in lines]),
                                              np.concatenate([part[2] for part in lines], axis=0), window_size=100000000)
        feat_enrich = lay.out("custom.enrich")
        with open(feat_enrich, "w") as fout:
            if ivals and not ids:       # intervals only: rows stay arrays end to end (millions of features)
                rows, rcounts = seqs.IntervalRows.concat([p_[0] for p_ in ivals]).merged(
                    np.concatenate([p_[1] for p_ in ivals], axis=0))
                sg_idx, _ = stats.enrich_ltr(fout, cl.d_sg, rcounts,
                                             colnames=cl.sg_names, rownames=rows, max_pval=self.max_pval, as_arrays=True)
                enriched = {i: cl.sg_names[j] for i, j in enumerate(sg_idx.tolist()) if j >= 0}
            else:
                for rows, cc in ivals:
                    ids = list(ids) + [(x, 0, 100000000) for x in rows.ids()]
                    counts = list(counts) + cc.tolist()
                if ivals:
                    # lines that share an id are ONE row whatever file they came from (Circos.stack_matrix,
                    # Circos.py:709-742, sums them): a BED interval listed twice, or listed next to a FASTA record of
                    # the same id, must give the row the intervals-only branch above gives (advisor r04)
                    merged = {}      # id -> summed row, in the order of the ids' first lines
                    for rid, row in zip(ids, counts):
                        merged[rid] = [x + y for x, y in zip(merged[rid], row)] if rid in merged else list(row)
                    ids, counts = list(merged), list(merged.values())
                enriched, _ = stats.enrich_ltr(fout, cl.d_sg, np.asarray(counts, np.int64).reshape(len(ids), S),
                                               colnames=cl.sg_names, rownames=ids, max_pval=self.max_pval)
        logger.info("wrote {}".format(feat_enrich))
        logger.info("{} significant subgenome-specific features".format(len(enriched)))
        for sg, n in sorted(Counter(enriched.values()).items()):
            logger.info("\t{} {}-specific features".format(n, sg))

    # ---- stage 6: homoeologous blocks ------------------------------------------------------------------------
    def stage_blocks(self, lay, labels, d_size, cl=None):
        """`blocks.tsv`, `block_link.txt` and `blocks.<figfmt>` from the anchor vote of every homoeologous pair (the pair
        list of Blocks.run_align over the config lines, or over -alt_cfgs).  A failure costs these files and nothing else."""
        for opt in ("aligner", "aligner_options"):
            if getattr(self, opt):
                logger.warning("-{} {}: no aligner is run; blocks come from shared single-copy k-mers".format(opt, getattr(self, opt)))
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            logger.info("blocks skipped: the stage runs on one GPU, this is a run of {} ranks".format(os.environ["WORLD_SIZE"]))
            return
        ctx = get_context()
        if not all(hasattr(ctx, m) for m in ("blocks_index", "blocks_pair", "blocks_release")):
            logger.info("blocks skipped: this context has no block entries")
            return
        try:
            sgs = self.sgs
            if self.alt_cfgs:      # another grouping for this stage only (__main__.py:280-286)
                rename = self.d_targets.get
                sgs = [[[rename(c, c) for c in unit] for unit in line]
                       for f in self.alt_cfgs for line in SGConfig(f, sep=self.sep).sgs]
            known = set(labels)
            lines = []
            for line in sgs:
                if len(line) < 2:
                    logger.info("blocks: config line {} has a single unit, no pair to compare".format(line))
                    lines.append([])
                    continue
                missing = sorted({c for unit in line for c in unit} - known)
                if missing:
                    logger.info("blocks: config line {} names chromosomes that are not loaded ({}), skipped".format(line, missing))
                    lines.append([])
                    continue
                lines.append(line)
            groups = blocks_mod.pair_list(lines)
            logger.info("###Step: Blocks")
            logger.info("homoeologous blocks of {} chromosome pairs (k = {}, 1 k-mer in {}, {}-bp windows)".format(
                sum(map(len, groups)), self.block_k, 1 << self.block_sample, self.block_bin))
            t0 = time.perf_counter()
            lengths = [d_size[lab] for lab in labels]
            res = blocks_mod.run(ctx, groups, labels, lengths, block_k=self.block_k, block_sample=self.block_sample,
                                 bin_size=self.block_bin, min_votes=self.block_votes, max_gap=self.block_gap,
                                 min_block=self.min_block)
            tsv, link, fig = lay.out("blocks.tsv"), lay.out("block_link.txt"), lay.out("blocks." + self.figfmt)
            with open(tsv, "w") as fout:
                blocks_mod.write_tsv(fout, [p for group in res for p in group])
            mk_ckp(lay.ckp(tsv))
            with open(link, "w") as fout:
                blocks_mod.write_links(fout, res)
            mk_ckp(lay.ckp(link))
            logger.info("blocks -> `{}` in {:.2f} s".format(os.path.basename(tsv), time.perf_counter() - t0))
        except Exception as e:
            logger.warning("blocks not written: {}".format(e))
            try:
                ctx.blocks_release()
            except Exception:
                pass
            return
        d_sg, sg_names = dict(getattr(cl, "d_sg", None) or {}), list(getattr(cl, "sg_names", None) or [])

        def draw():
            from matplotlib import pyplot as plt
            colors = self.colors or plt.rcParams["axes.prop_cycle"].by_key()["color"]
            chrom_colors = {c: colors[sg_names.index(sg) % len(colors)] for c, sg in d_sg.items() if sg in sg_names}
            blocks_mod.plot(fig, res, dict(zip(labels, lengths)), chrom_colors)
        self._plot_later(lay, "blocks", [fig], draw)

    # ---- stage 7: LTR-RTs from a .scn, or detected -----------------------------------------------------------
    def stage_ltr(self, lay, labels, cl, kmer_labels):
        """`.ltr.bin.count`, `.ltr.enrich`, `.ltr.identity.tsv`, `.ltr.insert.data`, `.ltr.insert.summary` and the two age
        figures from the LTR-RTs of -ltr_scn (step_ltr, __main__.py:549-620, without detection and classification), or from
        those -ltr_denovo detects and writes to `.ltr.scn`; with -ltr_tree the tree of the subgenome-specific ones."""
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            logger.info("LTR stage skipped: it runs on one GPU, this is a run of {} ranks".format(os.environ["WORLD_SIZE"]))
            return
        logger.info("###Step: LTR")
        ctx = get_context()
        band = int(self.ltr_band)
        if band < 0:
            raise ValueError("-ltr_band {} is below 0".format(band))
        self._ltr_tree_built = False
        want_tree = self.ltr_tree
        if want_tree and self.disable_ltrtree:
            logger.info("-disable_ltrtree: the LTR tree of -ltr_tree is not built")
            want_tree = False
        if want_tree and not all(hasattr(ctx, m) for m in ("ltr_sketch", "ltr_sketch_pairs", "nj_tree")):      # before anything is written
            raise RuntimeError("-ltr_tree needs a context with ltr_sketch, ltr_sketch_pairs and nj_tree (libsubphaser_hip.so); there "
                               "is no CPU engine for the tree")
        self._ltr_domtrees_built, self._ltr_dominfo = (), None
        want_domtree = self.ltr_domtree
        if want_domtree and self.disable_ltrtree:
            logger.info("-disable_ltrtree: the domain trees of -ltr_domtree are not built")
            want_domtree = False
        if want_domtree and not self.ltr_hmm:
            raise ValueError("-ltr_domtree builds its trees from the domains of the classification: give -ltr_hmm FILE as well")
        if want_domtree and not all(hasattr(ctx, m) for m in domtree_mod.REQUIRED):      # before anything is written
            raise RuntimeError("-ltr_domtree needs a context with dom_align, dom_peptide, aln_pairs and nj_tree (libsubphaser_hip.so); "
                               "there is no CPU engine for the domain trees")
        self._want_domtree = bool(want_domtree)
        if self.ltr_dom_prefilter is not None and not self.ltr_hmm:
            raise ValueError("-ltr_dom_prefilter filters the domain search of the classification: give -ltr_hmm FILE as well")
        self._ltr_profiles, self._ltr_clades = None, {}
        if self.ltr_hmm:
            if not hasattr(ctx, "dom_search"):      # before anything is written
                raise RuntimeError("-ltr_hmm needs a context with dom_search (libsubphaser_hip.so); there is no CPU engine for the "
                                   "domain search")
            self._ltr_profiles = domains_mod.read_hmm(self.ltr_hmm)
            if len(self._ltr_profiles) > domains_mod.MAX_P or max(self._ltr_profiles.M) > domains_mod.MAX_M:
                raise ValueError("{}: {} profiles of up to {} nodes; the domain search takes up to {} profiles of up to {} nodes".format(
                    self.ltr_hmm, len(self._ltr_profiles), max(self._ltr_profiles.M), domains_mod.MAX_P, domains_mod.MAX_M))
            logger.info("{} profiles of {}-{} nodes read from `{}`".format(len(self._ltr_profiles), min(self._ltr_profiles.M),
                                                                           max(self._ltr_profiles.M), self.ltr_hmm))
            if self.tesorter_options:
                logger.warning("-tesorter_options {}: TEsorter is not run; the domains come from this build's own search (-ltr_hmm, "
                               "-ltr_dom_cov, -ltr_dom_score)".format(self.tesorter_options))
            if self.intact_ltr:
                logger.info("-intact_ltr changes nothing, as in the reference: it is passed as intact_ltr= to a constructor whose "
                            "parameter is intact, and is lost")
        ltrs, chrom, st, en = self._ltr_records(lay, labels, ctx, band)
        d_enriched, d_exchange = self._ltr_enrich(lay, ctx, cl, kmer_labels, ltrs, chrom, st, en)
        ages = self._ltr_ages(lay, ctx, ltrs, chrom, band)
        if not d_enriched:
            logger.warning("Because of none subgenome-specific LTR-RTs, plots of LTR-RTs are skipped.")
            return
        dated = self._ltr_insert(lay, ltrs, ages, d_enriched, d_exchange, list(cl.sg_names))
        if dated and want_tree:
            self._ltr_tree(lay, ctx, ltrs, chrom, st, en, d_enriched, d_exchange, list(cl.sg_names))
        if dated and want_domtree:
            self._ltr_domtree(lay, ctx, ltrs, d_enriched, d_exchange, list(cl.sg_names))

    def _ltr_detected(self, lay, labels, ctx, band):
        """-ltr_denovo: (records, path) of the LTR-RTs ltr.detect finds, written to `.ltr.scn`; there is no CPU detector"""
        if not (hasattr(ctx, "ltr_seeds") and hasattr(ctx, "ltr_hsps") and hasattr(ctx, "ltr_align")):
            raise RuntimeError("-ltr_denovo needs a context with ltr_seeds, ltr_hsps and ltr_align (libsubphaser_hip.so); there is "
                               "no CPU detector: pass -ltr_scn FILE instead")
        opt = {name: getattr(self, "ltr_" + name) for name in ltr_mod.DETECT_OPTIONS}
        logger.info("Detecting LTR-RTs: seed {seed}, distance {mindist}-{maxdist}, LTR length {minlen}-{maxlen}, X-drop {xdrop}, "
                    "similarity >= {similar}, chaining {chain_indel} / {chain_join}; no TSD or motif search".format(**opt))
        ltrs, n = ltr_mod.detect(ctx, labels, band, opt)
        logger.info("{} seeds, {} extended seeds (HSPs), {} chains, {} candidates on {} chromosomes in {:.2f} s".format(
            n["seeds"], n["hsps"], n["chains"], n["candidates"], len(labels), n["t_seeds"]))
        if n["dropped"]:
            logger.info("{} candidates outside the limits of the alignment (band {}) or without an aligned column: dropped".format(n["dropped"], band))
        if n["candidates"]:
            logger.info("{} candidates aligned (band {}) in {:.2f} s; {} with similarity >= {}".format(
                n["candidates"], band, n["t_align"], len(ltrs), opt["similar"]))
        scn = lay.out("ltr.scn")
        with open(scn, "w") as fout:
            ltr_mod.write_scn(fout, ltrs)
        mk_ckp(lay.ckp(scn))
        logger.info("{} LTR-RTs detected, written to `{}`{}".format(len(ltrs), scn, self._ltr_unclassified_note()))
        return ltrs, scn

    _ltr_profiles, _ltr_clades = None, {}      # the profiles of -ltr_hmm and {id: clade} of the classified records (stage_ltr sets them)

    def _ltr_unclassified_note(self):
        return "" if self._ltr_profiles is not None else "; no classification: every record is used, as under -all_ltr"

    def _ltr_classify(self, lay, ctx, known, index):
        """-ltr_hmm: `.ltr.dom.gff3` and `.ltr.cls.tsv` of the records (LTRpipeline.classfify and the filter of LTRpipeline.run,
        LTR.py:335-361): the inner sequences, cut as get_int_seq cuts them, are searched on the device (Context.dom_search),
        domains.py turns the hits into domains and classes.  Returns (the records that stay, the keys of the complete ones)."""
        profiles, t0 = self._ltr_profiles, time.perf_counter()
        ival = [domains_mod.inner_interval(r) for r in known]
        long_ = [q for q, (a, b) in enumerate(ival) if b - a > domains_mod.MAX_LEN]
        if long_:
            logger.info("{} LTR-RTs with an inner sequence above {} bases are left unclassified".format(len(long_), domains_mod.MAX_LEN))
        pick = [q for q, (a, b) in enumerate(ival) if b - a <= domains_mod.MAX_LEN]
        pre, passed = {}, {}
        if self.ltr_dom_prefilter is not None:      # the ungapped prefilter: threshold in the search's units, 1/256 bit
            pre = dict(prefilter=int(math.ceil(float(self.ltr_dom_prefilter) * domains_mod.SCALE)), stats=passed)
        hits = np.asarray(ctx.dom_search(np.array([index[known[q].seq_id] for q in pick], np.int32), np.array([ival[q][0] for q in pick], np.int64),
                                         np.array([ival[q][1] for q in pick], np.int64), *profiles.tables(), **pre)) if pick else np.zeros((0, len(profiles), 6), np.int32)
        doms = domains_mod.best_domains([known[q].id for q in pick], [ival[q][1] - ival[q][0] for q in pick], hits, profiles,
                                        float(self.ltr_dom_cov), float(self.ltr_dom_score))
        rows = domains_mod.classify(doms)
        gff, cls = lay.out("ltr.dom.gff3"), lay.out("ltr.cls.tsv")
        with open(gff, "w") as fout:
            domains_mod.write_gff(fout, doms)
        mk_ckp(lay.ckp(gff))
        with open(cls, "w") as fout:
            domains_mod.write_cls(fout, rows)
        mk_ckp(lay.ckp(cls))
        note = ""
        if pre:
            items, kept_items = int(passed.get("items", 0)), int(passed.get("passed", 0))
            note = "; ungapped prefilter at {} bits: {} of {} (frame, profile) pairs ({:.2f}%) searched".format(
                self.ltr_dom_prefilter, kept_items, items, 1e2 * kept_items / items if items else 0.0)
        logger.info("{} inner sequences x {} profiles searched in {:.2f} s: {} domains (coverage >= {}, score >= {} bits per node) in {} "
                    "elements -> `{}`, `{}`{}".format(len(pick), len(profiles), time.perf_counter() - t0, len(doms), self.ltr_dom_cov,
                                                      self.ltr_dom_score, len(rows), os.path.basename(gff), os.path.basename(cls), note))
        if self._want_domtree:
            self._ltr_dominfo = dict(doms=doms, rows=rows, where={known[q].id: (index[known[q].seq_id],) + tuple(ival[q]) for q in pick})
            self._ltr_pep(lay, ctx)
        d_class = {r[0]: r for r in rows}
        kept, completed, n_ltr, n_intact = [], set(), 0, 0
        for r in known:
            row = d_class.get(domains_mod.format_gff_id(r.id))
            order, complete = (row[1], row[4]) if row else (None, None)
            n_ltr += order == "LTR"
            n_intact += complete == "yes"
            if not self.all_ltr and order != "LTR":
                continue
            kept.append(r)
            if row:
                self._ltr_clades[r.id] = row[3]
            if complete == "yes":
                completed.add(r.key)
        logger.info("By the device domain search, {} ({:.1%}) are classified as LTRs, of which {} ({:.1%}) are intact with complete protein "
                    "domains".format(n_ltr, n_ltr / max(1, len(known)), n_intact, n_intact / max(1, n_ltr)))
        return kept, completed

    def _ltr_records(self, lay, labels, ctx, band):
        """The elements the stage works on: read or detected, on target chromosomes, inside them, overlaps resolved, with their
        (chromosome index, start, end): the reference's seq[start:end], the Python slice taken with the 1-based start."""
        if self.ltr_denovo and not self.ltr_scn:
            ltrs, scn = self._ltr_detected(lay, labels, ctx, band)
        else:
            ltrs, scn = ltr_mod.read_scn(self.ltr_scn), self.ltr_scn
            logger.info("{} LTRs read from `{}`{}".format(len(ltrs), scn, self._ltr_unclassified_note()))
        index = {lab: i for i, lab in enumerate(labels)}
        known = []
        for r in ltrs:
            r.seq_id = self.d_targets.get(r.seq_id, r.seq_id)
            if r.seq_id in index:
                known.append(r)
        if len(known) < len(ltrs):
            logger.info("{} LTRs lie on sequences that are not target chromosomes: skipped".format(len(ltrs) - len(known)))
        lengths = [int(ctx.genome_len(i)) for i in range(len(labels))]
        for r in known:
            if not (1 <= r.start and r.lltr >= 1 and r.rltr >= 1 and r.lltr_e <= r.end and r.start <= r.rltr_s and r.end <= lengths[index[r.seq_id]]):
                raise ValueError("{}: LTR-RT {} does not lie on its chromosome (length {}) or its LTRs (lengths {}, {}) do not lie in it".format(
                    scn, r.id, lengths[index[r.seq_id]], r.lltr, r.rltr))
        kept, completed = known, None
        if self._ltr_profiles is not None:      # as LTRpipeline.run: classified before a record is dropped for overlap
            kept, completed = self._ltr_classify(lay, ctx, known, index)
        ltrs = ltr_mod.group_resolve_overlaps(kept, completed)
        logger.info("After filtering, {} / {} ({:.1%}) LTRs retained".format(len(ltrs), len(known), len(ltrs) / max(1, len(known))))
        chrom = np.array([index[r.seq_id] for r in ltrs], np.int32)
        st, en = np.array([r.start for r in ltrs], np.int64), np.array([r.end for r in ltrs], np.int64)
        if len(ltrs) and int((en - st).max()) > FEATURE_BIN:
            raise ValueError("{}: an LTR-RT of {} bases is longer than a {}-base bin".format(scn, int((en - st).max()), FEATURE_BIN))
        return ltrs, chrom, st, en

    def _ltr_enrich(self, lay, ctx, cl, kmer_labels, ltrs, chrom, st, en):
        """`.ltr.bin.count` (mapped elements only) and `.ltr.enrich`: ({id: subgenome} enriched, {id: "yes" / "no"} exchanged)"""
        S, names = len(cl.sg_names), list(cl.sg_names)
        ctx.labels_set(kmer_labels.keys, kmer_labels.sg_idx, S)
        counts = np.asarray(ctx.map_intervals(chrom, st, en), np.int64).reshape(len(ltrs), S) if len(ltrs) else np.zeros((0, S), np.int64)
        hit = np.flatnonzero(counts.sum(axis=1) > 0).tolist()
        ltr_map = lay.out("ltr.bin.count")
        logger.info("Outputing `coordinate` - `LTR` maps to `{}`".format(ltr_map))
        with open(ltr_map, "w") as fout:
            fout.write("\t".join(["#chrom", "start", "end"] + names) + "\n")
            for i in hit:
                fout.write("{}\t0\t{}\t{}\n".format(ltrs[i].id, int(en[i] - st[i]), "\t".join(map(str, counts[i].tolist()))))
        mk_ckp(lay.ckp(ltr_map))
        logger.info("Processed {} sequences".format(len(ltrs)))
        if len(ltrs) and len(kmer_labels.keys):
            logger.info("{} ({:.2%}) sequences contain subgenome-specific kmers".format(len(hit), len(hit) / len(ltrs)))
        logger.info("Enriching subgenome-specific LTR-RTs")
        ltr_enrich = lay.out("ltr.enrich")
        with open(ltr_enrich, "w") as fout:
            d_enriched, d_exchange = stats.enrich_ltr(fout, cl.d_sg, counts[hit], colnames=names, rownames=[ltrs[i].id for i in hit],
                                                      max_pval=self.max_pval, ctx=ctx)
        mk_ckp(lay.ckp(ltr_enrich))
        logger.info("Output: {}".format(ltr_enrich))
        logger.info("{} significant subgenome-specific LTR-RTs".format(len(d_enriched)))
        for sg, n in sorted(Counter(d_enriched.values()).items()):
            logger.info("\t{} {}-specific LTR-RTs".format(n, sg))
        return d_enriched, d_exchange

    def _ltr_ages(self, lay, ctx, ltrs, chrom, band):
        """`.ltr.identity.tsv`: the divergence of every element's two LTRs under -ltr_identity and its age at -mu; the ages"""
        mode, aligned = self.ltr_identity, None
        if not hasattr(ctx, "ltr_align"):
            if mode == "align":
                logger.info("this context has no ltr_align: -ltr_identity scn is used")
                mode = "scn"
        elif len(ltrs):
            t0 = time.perf_counter()
            a0, la, b0, lb = ltr_mod.ltr_intervals(ltrs)
            aligned = np.asarray(ctx.ltr_align(chrom, a0, la, b0, lb, band))
            logger.info("{} LTR pairs aligned (band {}) in {:.2f} s; {} touched the edge of their band".format(
                len(ltrs), band, time.perf_counter() - t0, int((aligned[:, 5] & ltr_mod.FLAG_EDGE != 0).sum())))
        divs, fell = ltr_mod.divergences(ltrs, aligned, mode)
        if mode == "align" and fell:
            logger.info("{} LTR pairs without an aligned substitution column or outside the limits of the alignment "
                        "take the similarity of the file".format(fell))
        ages = [ltr_mod.estimate_age(d, self.mu) for d in divs]
        ident = lay.out("ltr.identity.tsv")
        with open(ident, "w") as fout:
            ltr_mod.write_identity(fout, ltrs, aligned, divs, ages)
        mk_ckp(lay.ckp(ident))
        return ages

    def _ltr_insert(self, lay, ltrs, ages, d_enriched, d_exchange, sg_names):
        """`.ltr.insert.data`, `.ltr.insert.summary` and the two age figures; False: -exclude_exchanges left nothing to date"""
        prefix = lay.out("ltr.insert")
        with open(prefix + ".data", "w") as fout:
            d_data, _, excluded = ltr_mod.write_insert_data(fout, ltrs, ages, d_enriched, d_exchange,
                                                            exclude_exchanges=self.exclude_exchanges, non_specific=self.non_specific)
        if self.exclude_exchanges:
            logger.info("{} potentially exchanged LTR-RTs are excluded".format(excluded))
        if not d_data:      # every enriched element was excluded as an exchange
            logger.warning("no LTR-RT is left to date: `{}` and the plots are skipped".format(os.path.basename(prefix + ".summary")))
            return False
        with open(prefix + ".summary", "w") as fout:
            d_info = ltr_mod.summary_ltr_time(d_data, fout)
        mk_ckp(lay.ckp(prefix + ".summary"))
        figs = [prefix + ".density." + self.figfmt, prefix + ".histo." + self.figfmt]
        self._plot_later(lay, "LTR insertion ages", figs, lambda: ltr_mod.plot(d_data, d_info, figs[0], figs[1], self._sg_colors(sg_names)))
        return True

    def _ltr_tree(self, lay, ctx, ltrs, chrom, st, en, d_enriched, d_exchange, sg_names):
        """-ltr_tree: `.ltr.tree.nwk`, `.ltr.tree.map` and `.ltr.tree.<figfmt>` over the elements `.ltr.insert.data` lists as
        subgenome-specific (the reference's enrich_ltrs; without the exchanged ones under -exclude_exchanges).  The tree is this
        build's own object (ltrtree.py): sketches, Mash distances and neighbour joining on the device."""
        for opt in ("ggtree_options", "tree_method", "tree_options", "trimal_options", "ltr_domains"):
            if getattr(self, opt):
                logger.warning("-{} {}: no alignment or tree program is run; the tree comes from MinHash sketches and neighbour "
                               "joining".format(opt, getattr(self, opt)))
        k, s, limit, seed = int(self.ltr_tree_k), int(self.ltr_tree_sketch), int(self.subsample), self.bootstrap_seed
        if limit < 0:
            raise ValueError("-subsample {} is below 0".format(limit))
        picked = [i for i, r in enumerate(ltrs) if r.id in d_enriched and not (self.exclude_exchanges and d_exchange.get(r.id) == "yes")]
        too_long = [i for i in picked if en[i] - st[i] > ltrtree_mod.MAX_LEN]
        if too_long:
            logger.info("LTR tree: {} elements above {} bases are left out".format(len(too_long), ltrtree_mod.MAX_LEN))
            picked = [i for i in picked if en[i] - st[i] <= ltrtree_mod.MAX_LEN]
        cap = min(limit, ltrtree_mod.MAX_N) if limit else ltrtree_mod.MAX_N
        if len(picked) > cap:
            logger.info("LTR tree: {} of the {} subgenome-specific elements are kept (-subsample; at most {} in one tree)".format(
                cap, len(picked), ltrtree_mod.MAX_N))
            picked = [picked[q] for q in ltrtree_mod.choose(len(picked), cap, 0 if seed is None else seed)]
        if len(picked) < ltrtree_mod.MIN_SEQS:
            logger.info("LTR tree: {} subgenome-specific elements, fewer than {}: no tree".format(len(picked), ltrtree_mod.MIN_SEQS))
            return
        idx = np.array(picked, np.int64)
        ids, sgs = [ltrs[i].id for i in picked], [d_enriched[ltrs[i].id] for i in picked]
        records, (t_sk, t_pr, t_nj) = ltrtree_mod.build(ctx, chrom[idx], st[idx], en[idx], k, s)
        logger.info("LTR tree of {} elements (k = {}, {} hashes): sketches {:.2f} s, pairs {:.2f} s, neighbour joining {:.2f} s".format(
            len(picked), k, s, t_sk, t_pr, t_nj))
        nwk, tmap, fig = lay.out("ltr.tree.nwk"), lay.out("ltr.tree.map"), lay.out("ltr.tree." + self.figfmt)
        with open(nwk, "w") as fout:
            fout.write(ltrtree_mod.tree_text(records, ids) + "\n")
        mk_ckp(lay.ckp(nwk))
        with open(tmap, "w") as fout:
            ltrtree_mod.write_map(fout, ids, sgs, [self._ltr_clades.get(i, "unknown") for i in ids] if self._ltr_profiles is not None else None)
        mk_ckp(lay.ckp(tmap))
        logger.info("LTR tree -> `{}` (midpoint-rooted; one tree{})".format(
            os.path.basename(nwk), ", no clades: nothing is classified" if self._ltr_profiles is None else "; the Clade column is the domain classification's"))
        self._ltr_tree_built = True
        self._plot_later(lay, "LTR tree", [fig], lambda: ltrtree_mod.plot(fig, records, sgs, self._sg_colors(sg_names)))

    _want_domtree = False

    def _ltr_pep(self, lay, ctx):
        """-ltr_domtree: `.ltr.cls.pep`, the peptide of every line of `.ltr.dom.gff3` in the shape of TEsorter's `.cls.pep`"""
        info = self._ltr_dominfo
        doms, where = info["doms"], info["where"]
        place = [where[d.element] for d in doms]
        peps = domtree_mod.peptides_of(ctx, np.array([p[0] for p in place], np.int32), np.array([p[1] for p in place], np.int64),
                                       np.array([p[2] for p in place], np.int64), np.array([d.hit[0] for d in doms], np.int32),
                                       np.array([d.hit[1] for d in doms], np.int32), np.array([d.hit[2] for d in doms], np.int32))
        pep = lay.out("ltr.cls.pep")
        with open(pep, "w") as fout:
            domtree_mod.write_pep(fout, doms, info["rows"], peps)
        mk_ckp(lay.ckp(pep))
        logger.info("{} domain peptides -> `{}`".format(len(doms), os.path.basename(pep)))

    def _ltr_domtree(self, lay, ctx, ltrs, d_enriched, d_exchange, sg_names):
        """-ltr_domtree: per Copia / Gypsy `.ltr.LTR_<Superfamily>.aln`, `.map`, `.aln.trimmed`, `.aln.rooted.tre` and
        `.tree.<figfmt>` over the elements `.ltr.insert.data` lists as subgenome-specific (without the exchanged ones under
        -exclude_exchanges) that have every domain of -ltr_domains (LTR.LTRtree, LTR.py:144-233).  The trees are this build's
        own objects (domtree.py): profile alignment, occupancy trimming, Kimura distances and neighbour joining on the device."""
        if self.trimal_options:
            logger.warning("-trimal_options {}: trimal is not run; the columns of the domain alignments are kept by "
                           "-ltr_tree_occupancy {}".format(self.trimal_options, self.ltr_tree_occupancy))
        wanted = list(self.ltr_domains) if self.ltr_domains else list(domtree_mod.DOMAINS)
        limit, seed = int(self.subsample), self.bootstrap_seed
        occupancy, overlap = int(self.ltr_tree_occupancy), int(self.ltr_tree_overlap)
        if limit < 0:
            raise ValueError("-subsample {} is below 0".format(limit))
        if not 0 <= occupancy <= 100 or overlap < 0:
            raise ValueError("-ltr_tree_occupancy {} is outside 0..100 or -ltr_tree_overlap {} is below 0".format(occupancy, overlap))
        info, gid = self._ltr_dominfo, domains_mod.format_gff_id
        elem_domains = {}
        for d in info["doms"]:
            elem_domains.setdefault(d.element, {}).setdefault(d.gene, d)
        by_id = {x[0]: x for x in info["rows"]}
        classes = {r.id: (by_id[gid(r.id)][1], by_id[gid(r.id)][2]) for r in ltrs if gid(r.id) in by_id}
        candidates = [r.id for r in ltrs if r.id in d_enriched and not (self.exclude_exchanges and d_exchange.get(r.id) == "yes")]
        built = []
        for order, superfamily in domtree_mod.CATEGORIES:
            key = "{}_{}".format(order, superfamily)
            logger.info("Extracting and aligning protein domain sequences of {}/{}".format(order, superfamily))
            selected, counts = domtree_mod.select(candidates, elem_domains, classes, order, superfamily, wanted)
            for dom in wanted:
                logger.info("{} sequences contain {} domains".format(counts[dom], dom))
            logger.info("{} sequences contain all {} domains".format(len(selected), wanted))
            cap = min(limit, domtree_mod.MAX_N) if limit else domtree_mod.MAX_N
            if len(selected) > cap:
                logger.info("Subsample {} / {} ({:.2%})".format(cap, len(selected), cap / len(selected)))
                selected = [selected[q] for q in ltrtree_mod.choose(len(selected), cap, 0 if seed is None else seed)]
            t0 = time.perf_counter()
            kept_ids, blocks, common, left = domtree_mod.align_category(ctx, selected, elem_domains, info["where"], wanted, self._ltr_profiles) \
                if selected else ([], [[] for _ in wanted], {}, [])
            if left:
                logger.info("{}: {} elements with a window above {} residues are left out".format(key, len(left), domtree_mod.MAX_WIN))
            for dom in wanted:
                if dom in common:
                    logger.info("{}: {} is aligned to profile `{}`".format(key, dom, self._ltr_profiles.names[common[dom]]))
            t_align = time.perf_counter() - t0
            labels = [domtree_mod.format_id_for_iqtree(gid(e).split("#")[0]) for e in kept_ids]
            description, records, dropped = domtree_mod.cat_rows(labels, blocks, unique=True)
            aln, amap = lay.out("ltr.{}.aln".format(key)), lay.out("ltr.{}.map".format(key))
            with open(aln, "w") as fout:
                domtree_mod.write_aln(fout, records, description)
            mk_ckp(lay.ckp(aln), len(kept_ids))
            if kept_ids:
                logger.info("{} ({:.1%}) unique alignments retained".format(len(records), 1 - dropped / len(kept_ids)))
            else:
                logger.warning("0 sequences")
            with open(amap, "w") as fout:
                # every selected element, as the reference's: those left out for their window included
                ltrtree_mod.write_map(fout, [domtree_mod.format_id_for_iqtree(gid(e).split("#")[0]) for e in selected],
                                      [d_enriched[e] for e in selected], [self._ltr_clades.get(e, "unknown") for e in selected])
            mk_ckp(lay.ckp(amap))
            if len(records) < ltrtree_mod.MIN_SEQS:
                logger.info("{}: {} aligned rows, fewer than {}: no tree".format(key, len(records), ltrtree_mod.MIN_SEQS))
                continue
            names = [n for n, _ in records]
            trimmed = domtree_mod.trim([row for _, row in records], occupancy)
            trimfile = aln + ".trimmed"
            with open(trimfile, "w") as fout:
                domtree_mod.write_aln(fout, list(zip(names, trimmed)), description)
            mk_ckp(lay.ckp(trimfile))
            width = len(trimmed[0])
            if not 1 <= width <= domtree_mod.MAX_C:
                logger.info("{}: {} columns stay at -ltr_tree_occupancy {} (1 to {} are taken): no tree".format(key, width, occupancy, domtree_mod.MAX_C))
                continue
            t1 = time.perf_counter()
            same, both = ctx.aln_pairs(domtree_mod.encode(trimmed))
            D = domtree_mod.distance_matrix(same, both, overlap)
            t2 = time.perf_counter()
            records_nj = np.asarray(ctx.nj_tree(D), np.int64)
            logger.info("{} tree of {} rows x {} columns ({} before trimming): alignment {:.2f} s, pairs {:.2f} s, neighbour joining {:.2f} s".format(
                key, len(names), width, len(records[0][1]), t_align, t2 - t1, time.perf_counter() - t2))
            tre, fig = aln + ".rooted.tre", lay.out("ltr.{}.tree.{}".format(key, self.figfmt))
            with open(tre, "w") as fout:
                fout.write(ltrtree_mod.tree_text(records_nj, names) + "\n")
            mk_ckp(lay.ckp(tre))
            sg_of = dict(zip(labels, [d_enriched[e] for e in kept_ids]))
            sgs = [sg_of[n] for n in names]
            built.append(superfamily)
            self._plot_later(lay, "LTR {} domain tree".format(superfamily), [fig],
                             lambda fig=fig, rec=records_nj, sgs=sgs: ltrtree_mod.plot(fig, rec, sgs, self._sg_colors(sg_names)))
        self._ltr_domtrees_built = tuple(built)

    def run(self):
        self._reset()
        try:
            self._run()
        except BaseException:
            try:
                self._finish_background()      # do not leave writers behind; the stage's error is the one to report
            except Exception:
                pass
            raise
        self._finish_background()
        if self.cleanup:
            logger.info("Cleaning {}".format(self._lay.tmpdir))
            shutil.rmtree(self._lay.tmpdir, ignore_errors=True)
        logger.info("Pipeline completed" + (" early" if self.just_core else ""))

    def _run(self):
        lay = self._lay = Layout(self.outdir, self.tmpdir, self.prefix, self.k, self.min_freq, self.min_fold)
        chromfiles, labels, d_size, assigned = self.stage_ingest(lay)
        self.chromfiles, self.labels, self.d_size = chromfiles, labels, d_size
        d_mat2 = self.stage_count_filter(lay, chromfiles, labels)
        cl, kmer_labels = self.stage_cluster(lay, d_mat2, assigned)
        self.d_sg, self.sg_names = cl.d_sg, cl.sg_names
        if not self.just_core:
            self.stage_windows(lay, chromfiles, labels, d_size, cl, kmer_labels)
            if self.custom_features is not None:
                self._finish_background()      # `.kmer.mat` / sig-k-mer writers done: their threads would compete with the feature writers' 
                self.stage_features(lay, cl, kmer_labels)
            if not (self.disable_circos or self.disable_blocks):
                self.stage_blocks(lay, labels, d_size, cl)
            denovo = self.ltr_denovo and not self.ltr_scn
            if (self.ltr_scn or denovo) and not self.disable_ltr:
                self.stage_ltr(lay, labels, cl, kmer_labels)
                # the closing note: what of modules 3-4 this run did not do itself
                missing = (([] if denovo else ["LTR detection"]) + ([] if self.ltr_hmm else ["TEsorter classification"])
                           + ([] if self._ltr_tree_built or self._ltr_domtrees_built else ["the LTR trees"]))
                logger.info("Of modules 3-4, {}the circos figure {} not part of this build{}{}{}{}; run the reference on the outputs above "
                            "for {}".format(
                                ", ".join(missing) + " and " if missing else "", "are" if missing else "is",
                                "; the classification is this build's own Viterbi domain search (-ltr_hmm), not TEsorter's hmmscan"
                                if self.ltr_hmm else "",
                                " (the LTR-RTs are this build's own detection, not ltr_finder's or ltrharvest's)" if denovo else "",
                                "; the tree of -ltr_tree is this build's own (sketches and neighbour joining), not the reference's domain "
                                "trees" if self._ltr_tree_built else "",
                                "; the domain trees of -ltr_domtree ({}) are built and are this build's own (profile alignment, Kimura "
                                "distances, neighbour joining), not mafft / trimal / iqtree trees".format(", ".join(self._ltr_domtrees_built))
                                if self._ltr_domtrees_built else "", "them" if missing else "it"))
            elif not (self.disable_ltr and self.disable_circos):
                logger.info("Modules 3-4 (LTR, circos) are not part of this build; run the reference on the "
                            "outputs above, or pass -disable_ltr -disable_circos to silence this note")


for _dest, _default in option_defaults().items():
    setattr(Pipeline, _dest, _default)


def main(argv=None):
    args = makeArgparse(argv)
    if os.environ.get("SP_STACKS_AFTER"):      # debugging aid: dump every thread's Python stack after N seconds and exit
        import faulthandler
        faulthandler.dump_traceback_later(int(os.environ["SP_STACKS_AFTER"]), exit=True)
    logger.info("Command: {}".format(" ".join(sys.argv)))
    logger.info("Version: subphaser_amd {}".format(__version__))
    logger.info("Arguments: {}".format(args.__dict__))
    Pipeline(**args.__dict__).run()


def cli(argv=None):
    """Process entry point (`python -m subphaser_amd`, the `subphaser` script): main(), then leave without the interpreter's
    teardown.  When run() returns every output file is closed and every background writer joined; what is left is returning
    ~40 GB of device and page-locked memory buffer by buffer and unwinding numpy / matplotlib -- 1.1 of the 6.1 s of a
    wheat-sized run (profiles/r06_e2e_cli_wheat.log) that the operating system does in one piece when the process ends.
    `SP_SLOW_EXIT=1` keeps the ordinary exit (and, with `SP_EXIT_TRACE=1`, stamps its steps on stderr)."""
    main(argv)
    trace = bool(os.environ.get("SP_EXIT_TRACE"))
    if trace:
        sys.stderr.write("[exit] run() returned\n")
        sys.stderr.flush()
    if os.environ.get("SP_SLOW_EXIT") == "1":
        if trace:
            from .runtime import close_context
            close_context()
            sys.stderr.write("[exit] context closed\n")
            sys.stderr.flush()
        return
    import logging
    logging.shutdown()
    sys.stdout.flush()
    sys.stderr.flush()
    os._exit(0)


if __name__ == "__main__":
    cli()
