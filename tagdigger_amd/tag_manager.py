#!/usr/bin/env python3
"""Tag Manager, the reference's tag_manager.py: the same prompts on stdin / stdout (so it can be driven by piped
answers), the same files and printed lines.

    python -m tagdigger_amd.tag_manager [--td-device N] [--td-backend host]

Options 1-4: look up markers by sequence in a database, add a study's markers to a database (matching whole markers,
or consolidating markers that share tags), add alignment columns from a SAM file, start a new database.  The sorting,
lookups and tag comparisons run on the GPU (tagdigger_amd/tagset.py, csrc/tagset.hip); --td-backend host runs the
host restatement instead, with the same output.  Flags of this build only carry a --td- prefix.
"""
import argparse
import csv
import math
import sys

from . import tagdigger_fun


def build_parser():
    ap = argparse.ArgumentParser(description="TagDigger Tag Manager (MI355X build); answers are read from stdin")
    ap.add_argument('--td-device', type=int, default=0, help="GPU to run on (this build only)")
    ap.add_argument('--td-backend', choices=["gpu", "host"], default="gpu",
                    help="host: the host restatement of sorting, lookups and comparisons, no GPU (this build only)")
    return ap


def _yes_no(prompt, allowed=('Y', 'N')):
    answer = ''
    while answer not in set(allowed):
        answer = input(prompt).strip().upper()
    return answer


def _nonempty(prompt):
    answer = ''
    while answer == '':
        answer = input(prompt).strip()
    return answer


def _read_database():
    db = None
    while db == None:
        db = tagdigger_fun.readMarkerDatabase(input("Name of CSV file containing marker database: ").strip())
    return db


def _digits(text):
    return set(text) < set('0123456789')


def lookup(dev):
    """Option 1: look up markers in an existing database."""
    print("\nTags to look up in marker database:")
    tags = tagdigger_fun.readTags_interactive()
    db = _read_database()
    subset = _yes_no('Should markers be considered a match if only a subset of their tags match? (y/n) ')
    adl = _yes_no("Should tags be considered a match if one is a shorter version of the other? (y/n) ")
    print("Comparing tags...")
    compareDict = tagdigger_fun.compareTagSets(db[0], tags, perfectMatch=subset == 'N', allowDiffLengths=adl == 'Y', **dev)
    headers = db[1][0]
    extra = _yes_no('''Include additional columns from the database in the table?
a = include all, s = select which to include, n = include none: ''', ('A', 'S', 'N'))
    if extra == 'A':
        extracol = list(range(len(headers)))
    elif extra == 'N':
        extracol = []
    else:
        extracol = [i for i in range(len(headers)) if _yes_no("Include {}? (y/n) ".format(headers[i])) == 'Y']
    outfile = _nonempty("File name for CSV output: ")
    with open(outfile, 'w', newline='') as fh:
        out = csv.writer(fh)
        out.writerow(['Query', 'Marker name'] + [headers[i] for i in range(len(headers)) if i in extracol])
        for q in sorted(compareDict.keys()):
            if len(compareDict[q]) == 0:
                out.writerow([q, ''] + ['' for _ in extracol])
            for dbmarker in compareDict[q]:
                out.writerow([q, dbmarker] + [db[1][1][dbmarker][i] for i in range(len(headers)) if i in extracol])


def add_markers(dev):
    """Option 2: add a study's markers to an existing database."""
    print("\nNew tags to add to marker database:")
    tags = tagdigger_fun.readTags_interactive()
    allnew = tagdigger_fun.extractMarkers(tags[0])[0]
    db = _read_database()
    allold = sorted(db[1][1].keys())
    perfectMatch = _yes_no('Should markers be considered a match if only a subset of their tags match? (y/n) ') == 'N'
    adl = 'N' if perfectMatch else _yes_no(
        "Should tags be considered a match if one is a shorter version of the other? (y/n) ")
    inclOrig = _yes_no("Include column containing original marker names? (y/n) ")
    origColName = _nonempty("Column header for original marker names: ") if inclOrig == 'Y' else ""

    if perfectMatch:
        print("Comparing tags...")
        compareDict = tagdigger_fun.compareTagSets(db[0], tags, perfectMatch=True, allowDiffLengths=adl == 'Y', **dev)
        print("\nCounting markers...")
        matchedold = sorted([v[0] for v in compareDict.values() if len(v) == 1])
        nMrkr = len(allold) - len(matchedold) + len(allnew)
    else:
        nMrkr = len(allold) + len(allnew)
    minDig = math.ceil(math.log10(nMrkr))
    lastold = allold[-1]
    numDig = 0
    for i in range(1, len(lastold)):
        if lastold[-i] not in set('0123456789'):
            break
        numDig += 1
    Prefix = lastold[:-numDig]
    startingNum = int(lastold[-numDig:]) + 1

    print('Last marker name in existing database is {}.'.format(lastold))
    print('Prefix is {}, number of digits is {}, and new markers will be numbered starting {}.'.format(
        Prefix, numDig, startingNum))
    choice = input('\nPress enter to keep the prefix {}, or type different prefix to use with new markers: '.format(
        Prefix)).strip()
    if choice != '':
        Prefix = choice
    print('\nTotal number of markers is {}{}.'.format(nMrkr, "" if perfectMatch else " or less"))
    print('Minimum number of digits is {}.'.format(minDig))
    choice = 'a'
    while not _digits(choice) or numDig < minDig:
        choice = input('\nPress enter to keep {} as the number of digits, or enter a new number: '.format(numDig)).strip()
        if _digits(choice) and len(choice) > 0:
            numDig = int(choice)
    choice = 'a'
    while not _digits(choice) or "{}{:0{width}}".format(Prefix, startingNum, width=numDig) in allold:
        choice = input('\nPress enter to start numbering from {}, or enter a different starting number: '.format(
            startingNum)).strip()
        if _digits(choice) and len(choice) > 0:
            startingNum = int(choice)

    if perfectMatch:
        print("\nGenerating new marker names...")
        num = startingNum
        unmatchednew = []
        for m in allnew:
            if len(compareDict[m]) != 1:
                newname = "{}{:0{width}}".format(Prefix, num, width=numDig)
                num += 1
                unmatchednew.append(newname)
                compareDict[m] = [newname]
        print('{} out of {} markers are new.'.format(len(unmatchednew), len(allnew)))
        print("Adding new sequences to tag database...")
        fresh = set(unmatchednew)
        tagsNEW = [[], []]
        for t in range(len(tags[0])):
            tagname = tags[0][t]
            renamed = compareDict[tagname[:tagname.find('_')]][0]
            if renamed in fresh:
                tagsNEW[0].append(renamed + tagname[tagname.rfind('_'):])
                tagsNEW[1].append(tags[1][t])
    else:
        print("Consolidating old and new markers, and making new marker names...")
        alltags, compareDictRev = tagdigger_fun.consolidateTagSets(
            db[0], tags, allowDiffLengths=adl == 'Y', prefix=Prefix, numdig=numDig, startnumnew=startingNum, **dev)

    if _yes_no("Make FASTA file of new tags, to use with alignment software? (y/n): ") == 'Y':
        FAfile = _nonempty("Name for FASTA file: ")
        if not perfectMatch:
            first = "{}{:0{width}}".format(Prefix, startingNum, width=numDig) + "_"
            start = min([i for i in range(len(alltags[0])) if alltags[0][i].startswith(first)])
            tagsNEW = [alltags[0][start:], alltags[1][start:]]
        tagdigger_fun.exportFasta(FAfile, tagsNEW[0], tagsNEW[1], **dev)

    if _yes_no("\nAdd additional columns to database, referenced by original marker names? (y/n) ") == 'Y':
        if perfectMatch:
            markerDict = {k: compareDict[k][0] for k in compareDict.keys()}
        else:
            print("Preparing to match new names to original names...")
            markerDict = dict()
            newset = set(allnew)
            for k in compareDictRev.keys():
                for m in [x for x in compareDictRev[k] if x in newset]:
                    markerDict[m] = k
        addTable = None
        while addTable == None:
            addTable = tagdigger_fun.readTabularData(input("Name of CSV file with additional columns: ").strip(),
                                                     markerDict=markerDict)
        if len(set(addTable[0]) & set(db[1][0])) > 0:
            print('What should be done if conflicting data are found?')
            conflict = _yes_no('o = use old values, n = use new values :', ('O', 'N'))
            if conflict == 'O':
                combinedTables = tagdigger_fun.consolidateExtraCols([addTable, db[1]])
            else:
                combinedTables = tagdigger_fun.consolidateExtraCols([db[1], addTable])
        else:
            combinedTables = [db[1], addTable]
    else:
        combinedTables = [db[1]]

    outfile = _nonempty("\nName of CSV file for marker database output: ")
    if inclOrig == 'Y':
        if perfectMatch:
            combinedTables.append([[origColName], {compareDict[k][0]: [k] for k in compareDict.keys()}])
        else:
            combinedTables.append([[origColName], {k: [" ".join(compareDictRev[k])] for k in compareDictRev.keys()}])

    print('\nMaking merged tag sequences...')
    if perfectMatch:
        merged = tagdigger_fun.mergedTagList([db[0][0] + tagsNEW[0], db[0][1] + tagsNEW[1]], **dev)
    else:
        merged = tagdigger_fun.mergedTagList(alltags, **dev)
    if merged == None:
        print("Please check your input and then re-run the program.")
    else:
        print('Writing file...')
        tagdigger_fun.writeMarkerDatabase(outfile, merged[0], merged[1], combinedTables)


def add_alignments(dev):
    """Option 3: add alignment columns from a SAM file."""
    db = _read_database()
    if _yes_no("\nMake FASTA file of all tags, to use with alignment software? (y/n): ") == 'Y':
        FAfile = _nonempty("Name for FASTA file: ")
        tagdigger_fun.exportFasta(FAfile, db[0][0], db[0][1], **dev)
    sites = _yes_no("\nCalculate actual sites of SNPs, in addition to tag alignment position? (y/n): ") == 'Y'
    varDict = None
    if sites:
        print("Variable sites will only be output if there is a single variable site per marker.")
        varDict = tagdigger_fun.varSitesByMarker(db[0][0], db[0][1], **dev)
    bt = None
    while bt == None:
        bt = tagdigger_fun.readSAM(input("\nName of SAM file containing alignment data: ").strip(), varDict=varDict)
    colnames = [_nonempty('\nName for output column containing chromosome names: '),
                _nonempty('Name for output column containing alignment positions: '),
                _nonempty('Name for output column containing alignment qualities: ')]
    if sites:
        colnames.append(_nonempty('Name for output column containing variable site positions: '))
        btOut = dict()
        for k in bt.keys():
            row = bt[k]
            btOut[k] = list(row[0:3]) + [row[3][0] if len(row[3]) == 1 else ""]
    else:
        btOut = bt
    outfile = _nonempty("\nName of CSV file for marker database output: ")
    print('\nRemaking merged tag sequences...')
    merged = tagdigger_fun.mergedTagList(db[0], **dev)
    print('Writing file...')
    tagdigger_fun.writeMarkerDatabase(outfile, merged[0], merged[1], [db[1], [colnames, btOut]])


def new_database(dev):
    """Option 4: start a new database."""
    markers = None
    while markers == None:
        tags = tagdigger_fun.readTags_interactive()
        print("Creating merged tag strings for markers...\n")
        markers = tagdigger_fun.mergedTagList(tags, **dev)
    nMrkr = len(markers[0])
    minDig = math.ceil(math.log10(nMrkr))
    print('''Markers will be given names in the format Abcde000001.''')
    print('''It is recommended that marker names not include spaces.''')
    prefix = _nonempty('Prefix for marker names to output ("Abcde" in the above example): ')
    numDig = 0
    while numDig < minDig:
        numDig = int(input('Number of digits for numbering markers (6 in the above example): ').strip())
    names = ["{}{:0{width}}".format(prefix, i, width=numDig) for i in range(1, nMrkr + 1)]
    if _yes_no("Make FASTA file of tags to use with alignment software? (y/n): ") == 'Y':
        FAfile = _nonempty("Name for FASTA file: ")
        tagdigger_fun.exportFasta(FAfile, tags[0], tags[1], **dev)
    print('\nOptions for exporting SNP database:')
    inclOrig = _yes_no("Include column containing original marker names? (y/n) ")
    origColName = _nonempty("Column header for original marker names: ") if inclOrig == 'Y' else ""
    addTab = _yes_no("Add additional columns of data, referenced by original marker names? (y/n) ")
    addTable = None
    if addTab == 'Y':
        while addTable == None:
            addTable = tagdigger_fun.readTabularData(input("Name of CSV file with additional columns: ").strip(),
                                                     markerDict=dict(zip(markers[0], names)))
    extra = []
    if addTab == 'Y':
        extra.append(addTable)
    if inclOrig == 'Y':
        extra.append([[origColName], dict(zip(names, [[m] for m in markers[0]]))])
    outfile = _nonempty("Name of CSV file for marker database output: ")
    tagdigger_fun.writeMarkerDatabase(outfile, names, markers[1], extra)


def main(argv=None):
    args = build_parser().parse_args(argv)
    dev = {"device": args.td_device, "backend": args.td_backend}
    print('''
        TagDigger v. 1.1 Tag Manager
         Copyright Lindsay V. Clark
 Released under GNU General Public License v3
''')
    tagdigger_fun.set_directory_interactive()
    print('''
\tOptions are:
1. Look up markers by sequence in existing database
2. Add markers to existing database
3. Add alignment data to database
4. Start new database
''')
    which = "0"
    while which not in set('1234'):
        which = input("Select option: ").strip()
    {'1': lookup, '2': add_markers, '3': add_alignments, '4': new_database}[which](dev)
    input("\nPress enter to quit.")
    return 0


if __name__ == "__main__":
    sys.exit(main())
