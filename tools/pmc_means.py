"""Mean per dispatch of every counter of the fftlog kernel in rocprofv3 --pmc output directories, as JSON:  python tools/pmc_means.py DIR [DIR ...]"""
import collections
import csv
import glob
import json
import sys


def means(directory):
    acc = collections.defaultdict(list)
    for path in glob.glob('%s/**/*counter_collection.csv' % directory, recursive=True):
        with open(path) as f:
            for row in csv.DictReader(f):
                if 'fftlog' in row.get('Kernel_Name', ''):
                    acc[row['Counter_Name']].append(float(row['Counter_Value']))
    return {k: {'n_dispatches': len(v), 'mean': sum(v) / len(v)} for k, v in sorted(acc.items())}


if __name__ == '__main__':
    print(json.dumps({d: means(d) for d in sys.argv[1:]}, indent=1))
