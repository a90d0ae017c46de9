"""EPIC-Kitchens class tables (reference `core/dataset/epic_class.py:7-45`): same properties, same values.  The reference
reads the CSV again at every attribute access -- `get_info` asks four times per clip; here each file is read once, on
first use, and the result is kept."""
import ast
import os


class EpicClasses(object):
    """`EpicClasses(ann_path)`: `EPIC_verb_classes.csv`, `EPIC_noun_classes.csv` and `EPIC_many_shot_actions.csv` under
    `ann_path`.
      verbs / nouns      list of `class_key`, position = class id
      verb_df / noun_df  (`verb_id`, `verbs`) / (`noun_id`, `nouns`): the list-valued column exploded, one row per word
      actions            "verb noun" per row of the many-shot file"""

    def __init__(self, ann_path):
        self._ann_path = ann_path
        self._cache = {}

    def _csv(self, name):
        import pandas as pd
        key = ("csv", name)
        if key not in self._cache:
            self._cache[key] = pd.read_csv(os.path.join(self._ann_path, name))
        return self._cache[key]

    def _cached(self, key, make):
        if key not in self._cache:
            self._cache[key] = make()
        return self._cache[key]

    def _exploded(self, name, id_col, words_col):
        df = self._csv(name).copy()
        df[words_col] = df[words_col].apply(ast.literal_eval)
        return df.explode(words_col)[[id_col, words_col]]

    @property
    def verbs(self):
        return self._cached("verbs", lambda: self._csv("EPIC_verb_classes.csv").class_key.tolist())

    @property
    def nouns(self):
        return self._cached("nouns", lambda: self._csv("EPIC_noun_classes.csv").class_key.tolist())

    @property
    def verb_df(self):
        return self._cached("verb_df", lambda: self._exploded("EPIC_verb_classes.csv", "verb_id", "verbs"))

    @property
    def noun_df(self):
        return self._cached("noun_df", lambda: self._exploded("EPIC_noun_classes.csv", "noun_id", "nouns"))

    @property
    def actions(self):
        def make():
            df = self._csv("EPIC_many_shot_actions.csv")
            return df[["verb", "noun"]].agg(" ".join, axis=1).to_list()
        return self._cached("actions", make)
