#!/usr/bin/env python3
"""The interactive tag counter, the reference's tagdigger_interactive.py: the same prompts on stdin / stdout (so it can
be driven by piped answers), the same files and printed lines.

    python -m tagdigger_amd.tagdigger_interactive [--td-device N]

Asks for the cut site, the directory, a tag file in any of the seven formats and a key file ('File', 'Barcode',
'Sample'), counts every FASTQ file on the GPU (tagdigger_fun.find_tags_fastq), adds the libraries of each sample up and
writes the read counts and, for markers with alleles 0 and 1, diploid genotypes.  Flags of this build only carry a
--td- prefix.
"""
import argparse
import sys

from . import tagdigger_fun
from .barcode_splitter import CUTSITE_HELP, ask_cutsite, ask_keyfile, check_fastq, enzyme_table

BANNER = '''
                  TagDigger v. 1.1
             Copyright Lindsay V. Clark
    Released under GNU General Public License v3
    '''


def build_parser():
    ap = argparse.ArgumentParser(description="TagDigger (MI355X build); answers are read from stdin")
    ap.add_argument('--td-device', type=int, default=0, help="GPU to run on (this build only)")
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    print(BANNER)
    known = sorted(tagdigger_fun.enzymes.keys())
    print("Known restriction enzymes are:")
    print(enzyme_table(known))
    print(CUTSITE_HELP.format("ACGTRYSWKMBDHVN (IUPAC codes for ambiguous\nnucleotides)"))
    _, cutsite = ask_cutsite(known, 'ACGTRYSWKMBDHVN')
    print("Cut site: " + cutsite)

    tagdigger_fun.set_directory_interactive()
    tags = tagdigger_fun.readTags_interactive()
    tags = tagdigger_fun.sanitizeTags(tags)
    print("{} tag sequences remain.\n".format(len(tags[1])))

    bckeys = ask_keyfile("Name of key file with barcodes: ", strip=True)
    fqfiles = sorted(bckeys.keys())
    for f in fqfiles:
        print("File {}: {} barcodes".format(f, len(bckeys[f][0])))
    print("")
    bckeys, fqfiles = check_fastq(bckeys, fqfiles)

    countsfile = ""
    while countsfile == "":
        countsfile = input("\nFile name for output of read counts: ").strip()
    genofile = ""
    if set([t[-1] for t in tags[0]]) == {'0', '1'}:      # binary markers: offer numeric genotypes
        choice = ""
        while choice not in {'Y', 'N'}:
            choice = input("\nOutput CSV of diploid numeric genotypes? Y/N ").strip().upper()
        if choice == 'Y':
            while genofile == "":
                genofile = input("File name for output of genotypes: ").strip()

    input("\nPress enter to begin processing FASTQ files.")
    countsdict = dict()
    for f in fqfiles:
        countsdict[f] = tagdigger_fun.find_tags_fastq(f, bckeys[f][0], tags[1], cutsite=cutsite, device=args.td_device)
    combres = tagdigger_fun.combineReadCounts(countsdict, bckeys)
    tagdigger_fun.writeCounts(countsfile, combres[1], combres[0], tags[0])
    if genofile != "":
        tagdigger_fun.writeDiploidGeno(genofile, combres[1], combres[0], tags[0])

    input("\nPress enter to quit.")
    return 0


if __name__ == "__main__":
    sys.exit(main())
