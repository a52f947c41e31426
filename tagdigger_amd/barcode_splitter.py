#!/usr/bin/env python3
"""The interactive barcode splitter, the reference's barcode_splitter.py: the same prompts on stdin / stdout (so it can
be driven by piped answers), the same files and printed lines.

    python -m tagdigger_amd.barcode_splitter [--td-device N] [--td-backend host]

Asks for the cut site, the adapter set, the directory and a key file ('Input File', 'Barcode', 'Output File'), splits
every input file on the GPU (tagdigger_fun.barcodeSplitter) and, if asked, writes the MD5 checksums of the output files
(tagdigger_fun.writeMD5sums).  The checksums come from a pool of host threads, or from the GPU, one file per lane, for
lists as long as tagdigger_fun._MD5_DEVICE_MIN_FILES says; --td-backend host never uses the GPU for them.  The output
is the same either way.  Flags of this build only carry a --td- prefix.
"""
import argparse
import os
import sys

from . import tagdigger_fun

BANNER = '''
     TagDigger v. 1.1 Barcode Splitter
        Copyright Lindsay V. Clark
Released under GNU General Public License v3
'''
CUTSITE_HELP = '''
What restriction cut site should be found immediately
after the barcode sequence?  Type the name of one of the
above enzymes, OR type the restriction cut site as it
should appear in the sequence data (i.e. not including
bases before the beginning of the overhang) using
characters {}.
'''
RETRY_MENU = '''
Press 1 to re-read key file, 2 to search for FASTQ files in a different
directory, or 3 to try reading the same FASTQ files again: '''


def build_parser():
    ap = argparse.ArgumentParser(description="TagDigger barcode splitter (MI355X build); answers are read from stdin")
    ap.add_argument('--td-device', type=int, default=0, help="GPU to run on (this build only)")
    ap.add_argument('--td-backend', choices=["gpu", "host"], default="gpu",
                    help="host: MD5 checksums on host threads also for the long lists (384 files and more) that go to the GPU "
                         "otherwise (this build only)")
    return ap


def enzyme_table(names):
    """The names eight to a line, as one string."""
    return "".join(name + ("\n" if i % 8 == 7 else " ") for i, name in enumerate(names))


def ask_cutsite(known, alphabet):
    """(the answer as typed, the cut site): an enzyme's name or a site written in `alphabet`."""
    while True:
        choice = input("Restriction site: ")
        if choice in known:
            return choice, tagdigger_fun.enzymes[choice]
        if set(choice.upper()) <= set(alphabet):
            return choice, choice.upper()


def ask_keyfile(prompt, strip, **kwargs):
    keys = None
    while keys == None:
        name = input(prompt)
        keys = tagdigger_fun.readBarcodeKeyfile(name.strip() if strip else name, **kwargs)
    return keys


def check_fastq(bckeys, fqfiles):
    """The menu shown while some input file does not read as FASTQ; returns (bckeys, fqfiles) as they stand after it.
    Re-reading the key file here takes the counting columns and prints the length of the file's entry, as the
    reference's menu does."""
    fqok = [tagdigger_fun.isFastq(f) for f in fqfiles]
    while not all(fqok):
        print("Cannot read the following as FASTQ files:")
        for f, ok in zip(fqfiles, fqok):
            if not ok:
                print(f)
        choice = '0'
        while choice not in {'1', '2', '3'}:
            choice = input(RETRY_MENU).strip()
        if choice == '1':
            bckeys = ask_keyfile("\nName of key file with barcodes: ", strip=False)
            fqfiles = sorted(bckeys.keys())
            for f in fqfiles:
                print("File {}: {} barcodes".format(f, len(bckeys[f])))
            print("")
        if choice == '2':
            target = ""
            while not os.path.isdir(target):
                target = input("New directory: ")
            os.chdir(target)
        fqok = [tagdigger_fun.isFastq(f) for f in fqfiles]
    return bckeys, fqfiles


def main(argv=None):
    args = build_parser().parse_args(argv)
    print(BANNER)
    known = ["NsiI", "PstI"]
    print("Known restriction enzymes are:")
    print(enzyme_table(known))
    print(CUTSITE_HELP.format("ACGT"))
    enzchoice, cutsite = ask_cutsite(known, 'ACGT')
    print("Cut site: " + cutsite)

    print("\nKnown adapter sets:")
    adaptersets = sorted(tagdigger_fun.adapters.keys())
    for a in adaptersets:
        if enzchoice not in known or enzchoice in a:
            print(a)
    print("")
    adaptchoice = ""
    while adaptchoice not in adaptersets:
        adaptchoice = input("Choose an adapter set: ").strip()

    tagdigger_fun.set_directory_interactive()

    bckeys = ask_keyfile("\nName of key file with barcodes: ", strip=True, forSplitter=True)
    fqfiles = sorted(bckeys.keys())
    for f in fqfiles:
        print("File {}: {} barcodes".format(f, len(bckeys[f][0])))
    print("")
    bckeys, fqfiles = check_fastq(bckeys, fqfiles)

    print('')
    md5choice = ""
    while md5choice not in {'Y', 'N'}:
        md5choice = input("Create a CSV file of MD5 checksums? (y/n) ").strip().upper()
    md5outfile = ''
    if md5choice == 'Y':
        while md5outfile == '':
            md5outfile = input("Name of output CSV file to contain MD5 checksums: ").strip()

    input("\nPress enter to begin processing files.")
    for f in fqfiles:
        tagdigger_fun.barcodeSplitter(f, bckeys[f][0], bckeys[f][1], cutsite=cutsite,
                                      adapter=tagdigger_fun.adapters[adaptchoice], device=args.td_device)
    if md5choice == 'Y':
        filelist = []
        for f in fqfiles:
            filelist += bckeys[f][1]
        tagdigger_fun.writeMD5sums(filelist, md5outfile, device=args.td_device, backend=args.td_backend)

    input("\nPress enter to quit.")
    return 0


if __name__ == "__main__":
    sys.exit(main())
